// Steps through a time series the way Simian's key handler does (gluvv.cpp:970-1010) and draws each step with the
// host-side renderer mirror (HipVolumeRenderable::draw follows gluvv.volren.timestep, R8kVolRen3D.cpp:184-188).
// usage: timestep_main info <series.trex>
//          prints the MetaVolume series fields load_trex fills for every step (no GPU)
//        timestep_main draw <series.trex> <W> <H> <rate> <steps t0,t1,...> <out_prefix> [only=<t>]
//          init() at tstart, then per listed step: the key handler's work (swapTStep, else readAll + cacheTStep, here the
//          step's bricks swapped into the MetaVolume) and one draw(); frame k -> <out_prefix>.<k>.f32
//          [H][W][4] floats.  only=<t>: the series file's cache is ignored and step t is loaded, init()ed and drawn
//          alone: the frame of that step rendered on its own.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "HipVolumeRenderer.h"
#include "VolumeFiles.h"

gluvvGlobal gluvv;

static int write_frame(const std::string &path, const float *fb, size_t n) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return 1;
  const size_t w = fwrite(fb, 4, n, f);
  fclose(f);
  return w == n ? 0 : 1;
}

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  const std::string cmd = argv[1];
  std::string err;
  smkfiles::TrexHeader h;
  if (smkfiles::parse_trex(argv[2], &h, &err) != 1) {
    fprintf(stderr, "%s\n", err.c_str());
    return 5;
  }
  if (cmd == "info") {
    for (int t = h.tstart; t <= h.tstop; ++t) {
      smkfiles::LoadedVolume lv;
      if (!smkfiles::load_trex(argv[2], t, &lv, &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 5;
      }
      const MetaVolume &mv = lv.mv;
      printf("step=%d tsteps=%d tstart=%d tstop=%d tstepCache=%d currentTStep=%d file0=%s\n", t, mv.tsteps, mv.tstart, mv.tstop,
             mv.tstepCache, mv.currentTStep, smkfiles::brick_file(h, t, 0).c_str());
    }
    return 0;
  }
  if (cmd != "draw" || argc < 8) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);  // what initGluvv() does (gluvv.cpp:240-368)
  gluvv.win.width = atoi(argv[3]);
  gluvv.win.height = atoi(argv[4]);
  gluvv.volren.sampleRate = (float)atof(argv[5]);
  std::vector<int> steps;
  for (const char *p = argv[6]; *p;) {
    steps.push_back(atoi(p));
    while (*p && *p != ',') ++p;
    if (*p == ',') ++p;
  }
  const std::string prefix = argv[7];
  int only = -1;
  for (int a = 8; a < argc; ++a)
    if (std::string(argv[a]).rfind("only=", 0) == 0) only = atoi(argv[a] + 5);
  for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = (i % 5 == 0) ? 1.f : 0.f;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;

  // every step of the series read once (the host's disk reads; MetaVolume::readAll per step)
  std::vector<smkfiles::LoadedVolume> disk((size_t)(h.tstop - h.tstart + 1));
  for (int t = h.tstart; t <= h.tstop; ++t)
    if (!smkfiles::load_trex(argv[2], t, &disk[(size_t)(t - h.tstart)], &err)) {
      fprintf(stderr, "%s\n", err.c_str());
      return 5;
    }
  const int t0 = only >= 0 ? only : h.tstart;
  if (t0 < h.tstart || t0 > h.tstop) {
    fprintf(stderr, "step %d outside the series\n", t0);
    return 2;
  }
  // the MetaVolume Simian keeps: one object whose bricks' currentData the key handler swaps
  MetaVolume mv = disk[(size_t)(t0 - h.tstart)].mv;
  std::vector<Volume> vols = disk[(size_t)(t0 - h.tstart)].vols;
  mv.volumes = vols.data();
  if (only >= 0) mv.tstepCache = 0;
  gluvv.mv = &mv;
  gluvv.dmode = GDM_V1;
  gluvv.volren.timestep = t0;

  gluvvPrimitive renderables;  // "Dummy Node" list head (gluvv.cpp:252)
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  r->init();
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  TLUT *tl = gluvv.volren.tlut;  // VolumeRenderable::init's colour map: here an alpha ramp 0 -> .1
  for (int n = 0; n < tl->GetSize(); ++n) tl->GetRGBA(n)[3] = 0.1f * n / (tl->GetSize() - 1);
  gluvv.volren.loadTLUT = 1;
  const size_t npix = (size_t)gluvv.win.width * gluvv.win.height * 4;
  if (only >= 0) steps.assign(1, only);
  for (size_t k = 0; k < steps.size(); ++k) {
    const int t = steps[k];
    if (t < h.tstart || t > h.tstop) {
      fprintf(stderr, "step %d outside the series\n", t);
      return 2;
    }
    if (t != gluvv.volren.timestep) {  // '+' / '-' (gluvv.cpp:970-1010): the step lands in the MetaVolume, then a redisplay
      gluvv.volren.timestep = t;
      const smkfiles::LoadedVolume &d = disk[(size_t)(t - h.tstart)];
      for (int i = 0; i < mv.numSubVols; ++i) vols[(size_t)i].currentData = d.vols[(size_t)i].currentData;
      mv.currentTStep = t;
    }
    for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();  // display()
    if (!r->running()) return 4;
    if (write_frame(prefix + "." + std::to_string(k) + ".f32", r->framebuffer(), npix)) return 6;
  }
  delete r;
  return 0;
}
