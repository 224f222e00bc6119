// step_download_main.cpp -- the step the frames SHOW read back and saved through the host-side mirror: a series is played
// the way the key handler plays it (timestep_main.cpp), a fraction of time is set (HipVolumeRenderable::setTimeFraction), and
// the blend the frames then show is taken out of the renderer with HipVolumeRenderer::downloadStep and written to disk with
// HipVolumeRenderable::saveTimeStep -- what MetaVolume::writeAll (MetaVolume.cpp:963-1000) does from the host's arrays,
// for a step the host holds no array of.
// usage: step_download_main <nx ny nz nelts> <u16 0|1> <dmode> <t> <frac> <out prefix> <step files...>
//   every step file: [nz][ny][nx][nelts] voxels (uint16_t with u16 1), the series' steps 0, 1, ...; one draw() per step makes
//   them resident, then step t at fraction frac is shown and
//     <prefix>.data / .grad / .box  downloadStep's arrays and {origin[3], size[3]} as ints ("downloadStep <rc>" on stdout);
//     saveTimeStep(<prefix>.saved)  "<prefix>.saved.trex" + brick, or "<prefix>.saved.nrrd"   ("saveTimeStep <rc>" on stdout)
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

static bool spill(const std::string &p, const void *d, size_t n) {
  FILE *f = fopen(p.c_str(), "wb");
  if (!f) return false;
  const bool ok = fwrite(d, 1, n, f) == n;
  fclose(f);
  return ok;
}

int main(int argc, char **argv) {
  if (argc < 12) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);
  int a = 1;
  const int nx = atoi(argv[a++]), ny = atoi(argv[a++]), nz = atoi(argv[a++]), ne = atoi(argv[a++]);
  const bool u16 = atoi(argv[a++]) != 0;
  gluvv.dmode = (gluvvDataMode)atoi(argv[a++]);
  const int t = atoi(argv[a++]);
  const float frac = (float)atof(argv[a++]);
  const std::string out = argv[a++];
  std::vector<std::vector<unsigned char>> steps;
  for (; a < argc; ++a) {
    steps.push_back(slurp(argv[a]));
    if (steps.back().size() != (size_t)nx * ny * nz * ne * (u16 ? 2 : 1)) {
      fprintf(stderr, "%s: size mismatch\n", argv[a]);
      return 2;
    }
  }
  const int nsteps = (int)steps.size();
  if (t < 0 || t >= nsteps) {
    fprintf(stderr, "step %d outside the series\n", t);
    return 2;
  }
  // the MetaVolume Simian keeps: one brick whose currentData the key handler swaps, every step of the series cached
  MetaVolume mv;
  Volume v;
  const int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
  mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
  v.currentData = steps[0].data();
  mv.volumes = &v;
  mv.numSubVols = 1;
  mv.nelts = ne;
  mv.tsteps = nsteps;
  mv.tstart = 0;
  mv.tstop = nsteps - 1;
  mv.tstepCache = nsteps;
  gluvv.mv = &mv;
  gluvv.volren.timestep = 0;
  gluvv.win.width = gluvv.win.height = 16;
  gluvv.volren.sampleRate = 1.0f;
  for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = (i % 5 == 0) ? 1.f : 0.f;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;
  std::vector<unsigned char> dep((size_t)256 * 256 * 4, 40);  // a 2-D table: every voxel a little grey
  gluvv.volren.deptex = dep.data();

  gluvvPrimitive renderables;
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  r->useU16(u16 ? 1 : 0);
  r->init();
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  auto key = [&](int s) {  // '+' / '-' (gluvv.cpp:970-1010): the step lands in the MetaVolume, then a redisplay
    gluvv.volren.timestep = s;
    v.currentData = steps[(size_t)s].data();
    mv.currentTStep = s;
  };
  for (int s = 0; s < nsteps; ++s) {
    key(s);
    r->draw();
    if (!r->running()) return 4;
  }
  key(t);
  if (r->setTimeFraction(frac)) {
    fprintf(stderr, "setTimeFraction refused %g\n", (double)frac);
    return 7;
  }
  r->draw();
  if (!r->running()) return 4;

  std::vector<unsigned char> data, grad;
  int box[6] = {0, 0, 0, 0, 0, 0};
  const int rd = r->renderer()->downloadStep(&data, &grad, box, box + 3);
  printf("downloadStep %d\n", rd);
  if (rd && (!spill(out + ".data", data.data(), data.size()) || !spill(out + ".grad", grad.data(), grad.size()) ||
             !spill(out + ".box", box, sizeof box)))
    return 6;
  printf("saveTimeStep %d\n", r->saveTimeStep((out + ".saved").c_str()));
  delete r;
  return 0;
}
