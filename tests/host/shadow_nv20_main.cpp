// Drives the host-side mirror as a Simian session on a platform of its choice with gluvv.light.shadow on: on the GeForce3
// platform (GPNV20) that session draws with NV20VolRen3D2 (gluvv.cpp:151-159) -- the light buffer's opacity, with the ambient
// floor gluvv.light.amb --, on the Radeon 8500 one (GPATI8K) with R8kVolRen3D.  One draw(), the way display() does it; the
// float frame is written with the modelview the adapter built, so that a test can hand the C ABI the same state.
// usage: shadow_nv20_main <vol.u8 nx ny nz nelts> <grad.u8> <deptex.rgba> <W> <H> <rate> <xform16...> <lx ly lz> <buffer px>
//                         <quality> <platform: nv20 | r8k> <amb> <out prefix>
// writes <prefix>.f32 (the frame), <prefix>.mv (16 doubles)
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
  if (argc != 11 + 16 + 3 + 2 + 2 + 1) {
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
  // the GUI's shadow check box and quality spinner (gluvvui.cpp:150-167)
  gluvv.light.shadow = 1;
  gluvv.light.buffsz[0] = gluvv.light.buffsz[1] = atoi(argv[a++]);
  gluvv.light.gShadowQual = (float)atof(argv[a++]);
  // the platform (the card profile or the command line, gluvv.cpp:1230, 1463-1487), known before any renderer exists: it
  // decides which one starts (gluvv.cpp:141-199)
  const char *plat = argv[a++];
  if (!strcmp(plat, "nv20")) gluvv.plat = GPNV20;
  else if (!strcmp(plat, "r8k")) gluvv.plat = GPATI8K;
  else {
    fprintf(stderr, "platform must be nv20 or r8k\n");
    return 2;
  }
  gluvv.light.amb = (float)atof(argv[a++]);  // ("shadow strenght", gluvv.cpp:293)
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
  delete r;
  return bad ? 5 : 0;
}
