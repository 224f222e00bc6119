// Plays a time series at fractional times through the host-side renderer mirror (HipVolumeRenderable::setTimeFraction: the
// frames show the blend of the steps gluvv.volren.timestep and timestep + 1, made on the device by smk_blend_timesteps).
// usage: tblend_main frac|abi <series.trex> <W> <H> <rate> <t:f,t:f,...> <out_prefix>
//          init() at tstart and one draw() of every step of the series, so that the steps the series' cache holds are
//          resident; then per listed pair the key handler's work for step t (as timestep_main does it), the fraction f,
//          and one draw(); frame k -> <out_prefix>.<k>.f32, [H][W][4] floats, and a line
//          "frame <k> t=<t> f=<f> tblend_count=<blends the context has enqueued so far>" on stdout.
//          frac: the fraction goes to setTimeFraction.
//          abi:  the adapter stays on whole steps; a fraction > 0 is blended and selected through the C ABI on the
//                adapter's context, behind its back: the frame the adapter's own blend has to reproduce.
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
  if (argc < 8) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  const std::string cmd = argv[1];
  if (cmd != "frac" && cmd != "abi") {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  const bool abi = cmd == "abi";
  std::string err;
  smkfiles::TrexHeader h;
  if (smkfiles::parse_trex(argv[2], &h, &err) != 1) {
    fprintf(stderr, "%s\n", err.c_str());
    return 5;
  }
  gluvvCompatDefaults(gluvv);  // what initGluvv() does (gluvv.cpp:240-368)
  gluvv.win.width = atoi(argv[3]);
  gluvv.win.height = atoi(argv[4]);
  gluvv.volren.sampleRate = (float)atof(argv[5]);
  std::vector<std::pair<int, float>> seq;
  for (const char *p = argv[6]; *p;) {
    char *e = nullptr;
    const int t = (int)strtol(p, &e, 10);
    float f = 0;
    if (*e == ':') f = strtof(e + 1, &e);
    seq.push_back({t, f});
    p = e;
    while (*p && *p != ',') ++p;
    if (*p == ',') ++p;
  }
  const std::string prefix = argv[7];
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
  // the MetaVolume Simian keeps: one object whose bricks' currentData the key handler swaps
  MetaVolume mv = disk[0].mv;
  std::vector<Volume> vols = disk[0].vols;
  mv.volumes = vols.data();
  gluvv.mv = &mv;
  gluvv.dmode = GDM_V1;
  gluvv.volren.timestep = h.tstart;

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
  smk_ctx *c = r->renderer()->context();

  auto key = [&](int t) {  // '+' / '-' (gluvv.cpp:970-1010): the step lands in the MetaVolume, then a redisplay
    if (t == gluvv.volren.timestep) return;
    gluvv.volren.timestep = t;
    const smkfiles::LoadedVolume &d = disk[(size_t)(t - h.tstart)];
    for (int i = 0; i < mv.numSubVols; ++i) vols[(size_t)i].currentData = d.vols[(size_t)i].currentData;
    mv.currentTStep = t;
  };
  auto display = [&]() {
    for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();
    return r->running();
  };
  for (int t = h.tstart; t <= h.tstop; ++t) {
    key(t);
    if (!display()) return 4;
  }
  if (abi && smk_set_timestep_cache(c, (mv.tstepCache > 1 ? mv.tstepCache : 1) + 2)) {  // (room for the two outputs below)
    fprintf(stderr, "%s\n", smk_last_error(c));
    return 7;
  }
  for (size_t k = 0; k < seq.size(); ++k) {
    const int t = seq[k].first;
    const float f = seq[k].second;
    if (t < h.tstart || t > h.tstop) {
      fprintf(stderr, "step %d outside the series\n", t);
      return 2;
    }
    const bool moved = t != gluvv.volren.timestep;
    key(t);
    if (!abi) {
      if (r->setTimeFraction(f)) {
        fprintf(stderr, "setTimeFraction refused %g\n", (double)f);
        return 7;
      }
    } else if (f > 0) {
      const int id = 1000 + (int)(k & 1);
      if (moved && !display()) return 4;  // (the adapter selects the whole step; the blend then replaces it)
      if (smk_blend_timesteps(c, t, t + 1, f, id, nullptr) || smk_select_timestep(c, id)) {
        fprintf(stderr, "%s\n", smk_last_error(c));
        return 7;
      }
    } else if (!moved && smk_select_timestep(c, t)) {  // (back from a blend; a step that moved is the adapter's to select)
      fprintf(stderr, "%s\n", smk_last_error(c));
      return 7;
    }
    if (!display()) return 4;
    if (write_frame(prefix + "." + std::to_string(k) + ".f32", r->framebuffer(), npix)) return 6;
    double n = 0;
    smk_get_stat(c, "tblend_count", &n);
    printf("frame %zu t=%d f=%g tblend_count=%d\n", k, t, (double)f, (int)n);
  }
  delete r;
  return 0;
}
