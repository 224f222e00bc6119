// Plays a multi-field time series WITH H at fractional times with the derivatives of each blend (HipVolumeRenderable::
// setTimeFraction, setTimeFractionDerivatives and setBlurNormals: for a series of data mode GDM_V1GH or GDM_V2GH the frames
// show the blended fields with G and H of their summed gradient and its normals, blurred or plain, made on the device by
// smk_merge_timestep_h behind smk_blend_timesteps).
// usage: merge_h_main <series> <W> <H> <rate> <on|off> <blur|plain> <t:f,t:f,...> <out_prefix> [V2G|VGH]
//          <series>: "<prefix>:<nx>:<ny>:<nz>:<nelts>:<nsteps>:<deptex.rgba>[:<cache>]" -- the steps 0 .. nsteps - 1 a host
//                    prepared with mergeMV -addG -addH, "<prefix>.<t>.mf" [nz][ny][nx][nelts] bytes (nelts - 2 fields, G and H;
//                    nelts 3 or 4) and "<prefix>.<t>.nrm" [nz][ny][nx][3] normal bytes, <cache> of them kept resident
//                    (MetaVolume::tstepCache; default: all), under the 2-D table [256][256][4] of the seventh field.
//          init() at the first step and one draw() of every step of the series, so that the steps the series' cache holds are
//          resident; then per listed pair the key handler's work for step t, the fraction f, and one draw(); frame k ->
//          <out_prefix>.<k>.f32, [H][W][4] floats; the step that frame shows, read back (HipVolumeRenderer::downloadStep) ->
//          <out_prefix>.<k>.data and <out_prefix>.<k>.grad; and a line "frame <k> t=<t> f=<f>" on stdout.
//          on | off: setTimeFractionDerivatives.  blur | plain: setBlurNormals (plain leaves the setter alone).
//          V2G | VGH: a three-channel series of that data mode instead (two fields and G; V, G, H), for the setter's way
//          into smk_merge_timestep_h without H and into smk_derive_timestep.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "HipVolumeRenderer.h"

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
  if (argc < 9) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  const std::string series = argv[1], onoff = argv[5], blur = argv[6];
  if ((onoff != "on" && onoff != "off") || (blur != "blur" && blur != "plain")) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);  // what initGluvv() does (gluvv.cpp:240-368)
  gluvv.win.width = atoi(argv[2]);
  gluvv.win.height = atoi(argv[3]);
  gluvv.volren.sampleRate = (float)atof(argv[4]);
  std::vector<std::pair<int, float>> seq;
  for (const char *p = argv[7]; *p;) {
    char *e = nullptr;
    const int t = (int)strtol(p, &e, 10);
    float f = 0;
    if (*e == ':') f = strtof(e + 1, &e);
    seq.push_back({t, f});
    p = e;
    while (*p && *p != ',') ++p;
    if (*p == ',') ++p;
  }
  const std::string prefix = argv[8], other = argc > 9 ? argv[9] : "";
  if (other != "" && other != "V2G" && other != "VGH") {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = (i % 5 == 0) ? 1.f : 0.f;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;

  // every step of the series read once (the host's disk reads)
  std::vector<std::string> f;
  for (size_t a = 0;;) {
    const size_t b = series.find(':', a);
    f.push_back(series.substr(a, b == std::string::npos ? b : b - a));
    if (b == std::string::npos) break;
    a = b + 1;
  }
  if (f.size() != 7 && f.size() != 8) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  const int nx = atoi(f[1].c_str()), ny = atoi(f[2].c_str()), nz = atoi(f[3].c_str()), ne = atoi(f[4].c_str()), n = atoi(f[5].c_str());
  if (ne < 3 || ne > 4 || (other != "" && ne != 3)) {
    fprintf(stderr, "nelts %d: one or two fields, G and H\n", ne);
    return 2;
  }
  const size_t nvox = (size_t)nx * ny * nz;
  std::vector<std::vector<unsigned char>> vdata, vgrad;
  std::vector<unsigned char> dep = slurp(f[6]);
  for (int t = 0; t < n; ++t) {
    vdata.push_back(slurp(f[0] + "." + std::to_string(t) + ".mf"));
    vgrad.push_back(slurp(f[0] + "." + std::to_string(t) + ".nrm"));
    if (vdata.back().size() != nvox * (size_t)ne || vgrad.back().size() != nvox * 3 || !nvox) {
      fprintf(stderr, "step %d: size mismatch\n", t);
      return 5;
    }
  }
  if (n < 1 || dep.size() != 256 * 256 * 4) {
    fprintf(stderr, "no steps or no table\n");
    return 5;
  }
  MetaVolume mv;
  std::vector<Volume> vols;
  Volume v;
  const int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
  mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
  v.currentData = vdata[0].data();
  v.currentGrad = vgrad[0].data();
  vols.push_back(v);
  mv.numSubVols = 1;
  mv.nelts = ne;
  mv.tsteps = n;
  mv.tstart = 0;
  mv.tstop = n - 1;
  mv.tstepCache = f.size() == 8 ? atoi(f[7].c_str()) : n;
  gluvv.dmode = ne == 3 ? GDM_V1GH : GDM_V2GH;  // (what MetaVolume::mergeMV with -addH sets)
  if (other == "V2G") gluvv.dmode = GDM_V2G;
  if (other == "VGH") gluvv.dmode = GDM_VGH;
  gluvv.volren.deptex = dep.data();
  // the MetaVolume Simian keeps: one object whose bricks' currentData the key handler swaps
  mv.volumes = vols.data();
  gluvv.mv = &mv;
  gluvv.volren.timestep = 0;

  gluvvPrimitive renderables;  // "Dummy Node" list head (gluvv.cpp:252)
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  r->init();
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  const size_t npix = (size_t)gluvv.win.width * gluvv.win.height * 4;

  auto key = [&](int t) {  // '+' / '-' (gluvv.cpp:970-1010): the step lands in the MetaVolume, then a redisplay
    if (t == gluvv.volren.timestep) return;
    gluvv.volren.timestep = t;
    vols[0].currentData = vdata[(size_t)t].data();
    vols[0].currentGrad = vgrad[(size_t)t].data();
    mv.currentTStep = t;
  };
  auto display = [&]() {
    for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();
    return r->running();
  };
  for (int t = 0; t < n; ++t) {
    key(t);
    if (!display()) return 4;
  }
  r->setTimeFractionDerivatives(onoff == "on");
  if (blur == "blur") r->setBlurNormals(1);
  for (size_t k = 0; k < seq.size(); ++k) {
    const int t = seq[k].first;
    const float fq = seq[k].second;
    if (t < 0 || t >= n) {
      fprintf(stderr, "step %d outside the series\n", t);
      return 2;
    }
    key(t);
    if (r->setTimeFraction(fq)) {
      fprintf(stderr, "setTimeFraction refused %g\n", (double)fq);
      return 7;
    }
    if (!display()) return 4;
    const std::string out = prefix + "." + std::to_string(k);
    if (write_file(out + ".f32", r->framebuffer(), npix * sizeof(float))) return 6;
    std::vector<unsigned char> data, grad;
    if (!r->renderer()->downloadStep(&data, &grad, nullptr, nullptr)) return 8;
    if (write_file(out + ".data", data.data(), data.size()) || write_file(out + ".grad", grad.data(), grad.size())) return 6;
    printf("frame %zu t=%d f=%g\n", k, t, (double)fq);
  }
  delete r;
  return 0;
}
