// u16_adapter_main.cpp -- a 16-bit data set from disk through the host-side mirror, the way adapter_main drives the 8-bit
// one: VolumeFiles' load_trex (with keep16 when <u16> is 1) -> HipVolumeRenderable with useU16 -> init() -> draw().
// usage: u16_adapter_main <dataset.trex> <u16 0|1> <deptex.rgba> <W> <H> <rate> <xform16...> <out.f32>
//        a scalar data set under the 2-D table (gluvvDataMode V1 with gluvv.volren.deptex), unshaded
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "HipVolumeRenderer.h"
#include "VolumeFiles.h"

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

int main(int argc, char **argv) {
  if (argc != 7 + 16 + 1) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);  // what initGluvv() does (gluvv.cpp:240-368)
  const bool u16 = atoi(argv[2]) != 0;
  smkfiles::LoadedVolume loaded;
  std::string err;
  smkfiles::TrexHeader peek;
  if (smkfiles::parse_trex(argv[1], &peek, &err) != 1 || !smkfiles::load_trex(argv[1], peek.tstart, &loaded, &err, u16)) {
    fprintf(stderr, "%s\n", err.c_str());
    return 5;
  }
  auto dep = slurp(argv[3]);
  if (dep.empty()) return 2;
  int a = 4;
  gluvv.win.width = atoi(argv[a++]);
  gluvv.win.height = atoi(argv[a++]);
  gluvv.volren.sampleRate = (float)atof(argv[a++]);
  gluvv.shade = (gluvvShade)1;
  for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = (float)atof(argv[a++]);
  const char *out = argv[a++];
  gluvv.mv = &loaded.mv;
  gluvv.dmode = GDM_V1;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;
  gluvv.volren.deptex = dep.data();

  gluvvPrimitive renderables;  // "Dummy Node" list head (gluvv.cpp:252)
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  r->useU16(u16 ? 1 : 0);      // the switch: gluvv.mv's voxels are uint16_t and go up as SMK_U16
  renderables.setNext(r);
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->init();
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();
  if (!r->running()) return 4;
  FILE *f = fopen(out, "wb");
  if (!f) return 6;
  fwrite(r->framebuffer(), 4, (size_t)gluvv.win.width * gluvv.win.height * 4, f);
  fclose(f);
  delete r;
  return 0;
}
