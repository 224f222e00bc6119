// Drives the host-side mirror with the two switches a Simian session has on its perturbing renderer at once: gluvv.pert.on and
// gluvv.light.shadow (R8kVolRen3D_cpy: the noise texture bound in volShadow's eye pass and light pass alike).  One draw(), the way
// display() does it; the float frame is written with what the adapter was given beyond the arguments -- the modelview it built
// and the noise texture createNoiseTex makes (srand(1), libc rand) -- so that a test can hand the C ABI the same state.
// usage: shadow_perturb_main <vol.u8 nx ny nz nelts> <grad.u8> <deptex.rgba> <W> <H> <rate> <xform16...> <lx ly lz> <buffer px>
//                            <quality> <w0 w1 s0 s1> <out prefix>
// writes <prefix>.f32 (the frame), <prefix>.mv (16 doubles), <prefix>.noise (32^3 RGBA8)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "HipVolumeRenderer.h"

gluvvGlobal gluvv;

static std::vector<unsigned char> slurp(const char *p) {
  std::vector<unsigned char> v;
  FILE *f = fopen(p, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize(n);
  if (fread(v.data(), 1, n, f) != (size_t)n) v.clear();
  fclose(f);
  return v;
}

static int dump(const std::string &path, const void *p, size_t bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return 1;
  const size_t n = fwrite(p, 1, bytes, f);
  fclose(f);
  return n != bytes;
}

int main(int argc, char **argv) {
  if (argc != 11 + 16 + 3 + 2 + 4 + 1) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);  // what initGluvv() does (gluvv.cpp:240-368)
  int a = 1;
  auto vol = slurp(argv[a++]);
  int nx = atoi(argv[a++]), ny = atoi(argv[a++]), nz = atoi(argv[a++]), ne = atoi(argv[a++]);
  auto grad = slurp(argv[a++]);
  auto dep = slurp(argv[a++]);
  gluvv.win.width = atoi(argv[a++]);
  gluvv.win.height = atoi(argv[a++]);
  gluvv.volren.sampleRate = gluvv.volren.goodSamp = (float)atof(argv[a++]);  // (the good rate in force: gShadowQual applies)
  gluvv.shade = gluvvShadeDSpec;
  for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = (float)atof(argv[a++]);
  for (int i = 0; i < 3; ++i) gluvv.light.pos[i] = (float)atof(argv[a++]);
  // the GUI's shadow check box and quality spinner (gluvvui.cpp:150-167), and its perturbation roll-out (:213-267)
  gluvv.light.shadow = 1;
  gluvv.light.buffsz[0] = gluvv.light.buffsz[1] = atoi(argv[a++]);
  gluvv.light.gShadowQual = (float)atof(argv[a++]);
  gluvv.pert.on = 1;
  gluvv.pert.weights[0] = (float)atof(argv[a++]);
  gluvv.pert.weights[1] = (float)atof(argv[a++]);
  gluvv.pert.scales[0] = (float)atof(argv[a++]);
  gluvv.pert.scales[1] = (float)atof(argv[a++]);
  const std::string out = argv[a++];
  if (vol.size() != (size_t)nx * ny * nz * ne || grad.empty() || dep.empty()) {
    fprintf(stderr, "volume size mismatch, or no gradient / table\n");
    return 2;
  }
  MetaVolume mv;  // as the loader leaves it: one brick, largest dimension normalised to 1
  Volume v;
  int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
  mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
  v.currentData = vol.data();
  v.currentGrad = grad.data();
  mv.volumes = &v;
  mv.numSubVols = 1;
  mv.nelts = ne;
  gluvv.mv = &mv;
  gluvv.dmode = GDM_VGH;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;
  gluvv.volren.deptex = dep.data();

  gluvvPrimitive renderables;  // "Dummy Node" list head (gluvv.cpp:252)
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->init();  // initRenderables
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();  // display()
  if (!r->running() || !r->renderer()->ok()) return 4;
  int bad = dump(out + ".f32", r->framebuffer(), (size_t)gluvv.win.width * gluvv.win.height * 16);
  double mvm[16];
  HipVolumeRenderable::modelview(mvm);
  bad |= dump(out + ".mv", mvm, sizeof mvm);
  // R8kVolRen3D_cpy::createNoiseTex (:2392-2436) as the adapter's init() runs it: srand(1), four draws per texel
  std::vector<unsigned char> noise((size_t)32 * 32 * 32 * 4);
  srand(1);
  for (size_t q = 0; q < noise.size(); ++q) noise[q] = (unsigned char)(((rand() / (float)RAND_MAX * .5) + .5 + 1.0 / 512) * 255);
  bad |= dump(out + ".noise", noise.data(), noise.size());
  delete r;
  return bad ? 5 : 0;
}
