// Drives the host-side mirror for a few frames the way Simian's display() does (gluvv.cpp:518-525, 593-623) and writes what a
// host would hand to glDrawPixels: the float frames of two poses (the default mode), then the same two poses through the
// pipelined present mode (a draw() hands over the frame of the draw() before it), then through the synchronous one.
// usage: present_main <vol.u8 nx ny nz nelts> <grad.u8|-> <deptex.rgba|-> <W> <H> <rate> <shade 0|3> <xformA16...> <xformB16...>
//                     <bgColor> <out prefix>
// writes <prefix>.a.f32 .b.f32 (float frames of pose A, B), .p1.rgba8 .p2.rgba8 .p3.rgba8 (pipelined: after draw A, after draw
// B, after flush()) with .p2.zwin .p3.zwin, and .s1.rgba8 .s2.rgba8 .s2.zwin (synchronous: after draw A, after draw B)
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
  if (!p) {
    fprintf(stderr, "%s: no buffer\n", path.c_str());
    return 1;
  }
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return 1;
  const size_t n = fwrite(p, 1, bytes, f);
  fclose(f);
  return n != bytes;
}

int main(int argc, char **argv) {
  if (argc != 12 + 16 + 16 + 2) {
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
  gluvv.volren.sampleRate = (float)atof(argv[a++]);
  gluvv.shade = (gluvvShade)atoi(argv[a++]);
  float pose[2][16];
  for (int p = 0; p < 2; ++p)
    for (int i = 0; i < 16; ++i) pose[p][i] = (float)atof(argv[a++]);
  gluvv.env.bgColor = atoi(argv[a++]);
  const std::string out = argv[a++];
  if (vol.size() != (size_t)nx * ny * nz * ne) {
    fprintf(stderr, "volume size mismatch\n");
    return 2;
  }
  MetaVolume mv;  // as the loader leaves it: one brick, largest dimension normalised to 1
  Volume v;
  int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
  mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
  v.currentData = vol.data();
  v.currentGrad = grad.empty() ? nullptr : grad.data();
  mv.volumes = &v;
  mv.numSubVols = 1;
  mv.nelts = ne;
  gluvv.mv = &mv;
  gluvv.dmode = ne == 1 ? GDM_V1 : GDM_VGH;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;
  if (!dep.empty()) gluvv.volren.deptex = dep.data();

  gluvvPrimitive renderables;  // "Dummy Node" list head (gluvv.cpp:252)
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->init();  // initRenderables
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  if (ne == 1) {  // VolumeRenderable::init's colour map: here a plain alpha ramp 0 -> .1
    TLUT *t = gluvv.volren.tlut;
    for (int n = 0; n < t->GetSize(); ++n) t->GetRGBA(n)[3] = 0.1f * n / (t->GetSize() - 1);
    gluvv.volren.loadTLUT = 1;
  }
  const size_t npix = (size_t)gluvv.win.width * gluvv.win.height;
  auto draw = [&](int p) {  // display(): the pose the mouse left, then every renderable
    for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = pose[p][i];
    for (gluvvPrimitive *q = renderables.getNext(); q; q = q->getNext()) q->draw();
    return r->running();
  };
  int bad = 0;
  // the float frames (the default mode: one draw() one frame)
  if (!draw(0)) return 4;
  bad |= dump(out + ".a.f32", r->framebuffer(), npix * 16);
  if (!draw(1)) return 4;
  bad |= dump(out + ".b.f32", r->framebuffer(), npix * 16);
  // pipelined: draw() enqueues its frame and hands over the one before it
  r->present(HipPresentPipelined, 1);
  if (!draw(0)) return 4;
  bad |= dump(out + ".p1.rgba8", r->framebuffer8(), npix * 4);  // (nothing has arrived yet: the cleared frame)
  if (!draw(1)) return 4;
  bad |= dump(out + ".p2.rgba8", r->framebuffer8(), npix * 4);  // pose A
  bad |= dump(out + ".p2.zwin", r->depthbuffer(), npix * 4);
  r->flush();
  bad |= dump(out + ".p3.rgba8", r->framebuffer8(), npix * 4);  // pose B
  bad |= dump(out + ".p3.zwin", r->depthbuffer(), npix * 4);
  // synchronous: one draw() one frame
  r->present(HipPresentSync, 1);
  if (!draw(0)) return 4;
  bad |= dump(out + ".s1.rgba8", r->framebuffer8(), npix * 4);
  if (!draw(1)) return 4;
  bad |= dump(out + ".s2.rgba8", r->framebuffer8(), npix * 4);
  bad |= dump(out + ".s2.zwin", r->depthbuffer(), npix * 4);
  if (!r->running() || !r->renderer()->ok()) return 4;
  delete r;
  return bad ? 5 : 0;
}
