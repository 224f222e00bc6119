// Plays a time series at fractional times with the derivatives of each blend (HipVolumeRenderable::setTimeFraction and
// setTimeFractionDerivatives: the frames show V, G, H and normals of the blended scalar, made on the device by
// smk_derive_timestep behind smk_blend_timesteps).
// usage: derive_main <series> <W> <H> <rate> <on|off> <t:f,t:f,...> <out_prefix>
//          <series>: a scalar series "<name>.trex" (as tblend_main reads it: one channel, the 1-D colour map), or
//                    "vgh:<prefix>:<nx>:<ny>:<nz>:<nsteps>:<deptex.rgba>[:<cache>]" -- the V, G, H steps 0 .. nsteps - 1 a host
//                    prepared, "<prefix>.<t>.vgh" [nz][ny][nx][3] bytes and "<prefix>.<t>.nrm" [nz][ny][nx][3] normal bytes,
//                    <cache> of them kept resident (MetaVolume::tstepCache; default: all), under the 2-D table
//                    [256][256][4] of the sixth field.
//          init() at the first step and one draw() of every step of the series, so that the steps the series' cache holds are
//          resident; then per listed pair the key handler's work for step t, the fraction f, and one draw(); frame k ->
//          <out_prefix>.<k>.f32, [H][W][4] floats; the step that frame shows, read back (HipVolumeRenderer::downloadStep) ->
//          <out_prefix>.<k>.data and <out_prefix>.<k>.grad; and a line
//          "frame <k> t=<t> f=<f> tblend_count=<blends the context has enqueued so far>" on stdout.
//          on | off: setTimeFractionDerivatives.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "HipVolumeRenderer.h"
#include "VolumeFiles.h"

gluvvGlobal gluvv;

static int write_file(const std::string &path, const void *p, size_t bytes) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return 1;
  const size_t w = fwrite(p, 1, bytes, f);
  fclose(f);
  return w == bytes ? 0 : 1;
}

static std::vector<unsigned char> slurp(const std::string &path) {
  std::vector<unsigned char> b;
  FILE *f = fopen(path.c_str(), "rb");
  if (!f) return b;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  b.resize(n > 0 ? (size_t)n : 0);
  if (n > 0 && fread(b.data(), 1, (size_t)n, f) != (size_t)n) b.clear();
  fclose(f);
  return b;
}

int main(int argc, char **argv) {
  if (argc < 8) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  const std::string series = argv[1], onoff = argv[5];
  if (onoff != "on" && onoff != "off") {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);  // what initGluvv() does (gluvv.cpp:240-368)
  gluvv.win.width = atoi(argv[2]);
  gluvv.win.height = atoi(argv[3]);
  gluvv.volren.sampleRate = (float)atof(argv[4]);
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

  // every step of the series read once (the host's disk reads)
  const bool vgh = series.compare(0, 4, "vgh:") == 0;
  int tstart = 0, tstop = 0;
  std::vector<smkfiles::LoadedVolume> disk;               // the scalar series
  std::vector<std::vector<unsigned char>> vdata, vgrad;   // the V, G, H series
  std::vector<unsigned char> dep;
  MetaVolume mv;
  std::vector<Volume> vols;
  if (!vgh) {
    std::string err;
    smkfiles::TrexHeader h;
    if (smkfiles::parse_trex(series.c_str(), &h, &err) != 1) {
      fprintf(stderr, "%s\n", err.c_str());
      return 5;
    }
    tstart = h.tstart;
    tstop = h.tstop;
    disk.resize((size_t)(tstop - tstart + 1));
    for (int t = tstart; t <= tstop; ++t)
      if (!smkfiles::load_trex(series.c_str(), t, &disk[(size_t)(t - tstart)], &err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 5;
      }
    mv = disk[0].mv;
    vols = disk[0].vols;
    gluvv.dmode = GDM_V1;
  } else {
    std::vector<std::string> f;
    for (size_t a = 4;;) {
      const size_t b = series.find(':', a);
      f.push_back(series.substr(a, b == std::string::npos ? b : b - a));
      if (b == std::string::npos) break;
      a = b + 1;
    }
    if (f.size() != 6 && f.size() != 7) {
      fprintf(stderr, "bad usage\n");
      return 2;
    }
    const int nx = atoi(f[1].c_str()), ny = atoi(f[2].c_str()), nz = atoi(f[3].c_str()), n = atoi(f[4].c_str());
    const size_t bytes = (size_t)nx * ny * nz * 3;
    dep = slurp(f[5]);
    for (int t = 0; t < n; ++t) {
      vdata.push_back(slurp(f[0] + "." + std::to_string(t) + ".vgh"));
      vgrad.push_back(slurp(f[0] + "." + std::to_string(t) + ".nrm"));
      if (vdata.back().size() != bytes || vgrad.back().size() != bytes || !bytes) {
        fprintf(stderr, "step %d: size mismatch\n", t);
        return 5;
      }
    }
    if (n < 1 || dep.size() != 256 * 256 * 4) {
      fprintf(stderr, "no steps or no table\n");
      return 5;
    }
    tstop = n - 1;
    Volume v;
    const int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
    mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
    mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
    v.currentData = vdata[0].data();
    v.currentGrad = vgrad[0].data();
    vols.push_back(v);
    mv.numSubVols = 1;
    mv.nelts = 3;
    mv.tsteps = n;
    mv.tstart = 0;
    mv.tstop = n - 1;
    mv.tstepCache = f.size() == 7 ? atoi(f[6].c_str()) : n;
    gluvv.dmode = GDM_VGH;
    gluvv.volren.deptex = dep.data();
  }
  // the MetaVolume Simian keeps: one object whose bricks' currentData the key handler swaps
  mv.volumes = vols.data();
  gluvv.mv = &mv;
  gluvv.volren.timestep = tstart;

  gluvvPrimitive renderables;  // "Dummy Node" list head (gluvv.cpp:252)
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  r->init();
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  if (!vgh) {
    TLUT *tl = gluvv.volren.tlut;  // VolumeRenderable::init's colour map: here an alpha ramp 0 -> .1, as tblend_main's
    for (int n = 0; n < tl->GetSize(); ++n) tl->GetRGBA(n)[3] = 0.1f * n / (tl->GetSize() - 1);
    gluvv.volren.loadTLUT = 1;
  }
  const size_t npix = (size_t)gluvv.win.width * gluvv.win.height * 4;
  smk_ctx *c = r->renderer()->context();

  auto key = [&](int t) {  // '+' / '-' (gluvv.cpp:970-1010): the step lands in the MetaVolume, then a redisplay
    if (t == gluvv.volren.timestep) return;
    gluvv.volren.timestep = t;
    if (vgh) {
      vols[0].currentData = vdata[(size_t)t].data();
      vols[0].currentGrad = vgrad[(size_t)t].data();
    } else {
      const smkfiles::LoadedVolume &d = disk[(size_t)(t - tstart)];
      for (int i = 0; i < mv.numSubVols; ++i) vols[(size_t)i].currentData = d.vols[(size_t)i].currentData;
    }
    mv.currentTStep = t;
  };
  auto display = [&]() {
    for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();
    return r->running();
  };
  for (int t = tstart; t <= tstop; ++t) {
    key(t);
    if (!display()) return 4;
  }
  r->setTimeFractionDerivatives(onoff == "on");
  for (size_t k = 0; k < seq.size(); ++k) {
    const int t = seq[k].first;
    const float f = seq[k].second;
    if (t < tstart || t > tstop) {
      fprintf(stderr, "step %d outside the series\n", t);
      return 2;
    }
    key(t);
    if (r->setTimeFraction(f)) {
      fprintf(stderr, "setTimeFraction refused %g\n", (double)f);
      return 7;
    }
    if (!display()) return 4;
    const std::string out = prefix + "." + std::to_string(k);
    if (write_file(out + ".f32", r->framebuffer(), npix * sizeof(float))) return 6;
    std::vector<unsigned char> data, grad;
    if (!r->renderer()->downloadStep(&data, &grad, nullptr, nullptr)) return 8;
    if (write_file(out + ".data", data.data(), data.size()) || write_file(out + ".grad", grad.data(), grad.size())) return 6;
    double n = 0;
    smk_get_stat(c, "tblend_count", &n);
    printf("frame %zu t=%d f=%g tblend_count=%d\n", k, t, (double)f, (int)n);
  }
  delete r;
  return 0;
}
