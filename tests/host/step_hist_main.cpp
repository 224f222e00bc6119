// step_hist_main.cpp -- the transfer-function window's two readers of the data, through the host-side mirror: the joint
// histogram behind the widgets (TFWidgetRen::loadHist, TFWidgetRen1.cpp:660-700) and the data probe (TFWidgetRen::drawProbe,
// :309-595), both taken from the step the renderer SHOWS (HipVolumeRenderer::hist2DStep / probeStep) and, where the host
// holds bytes, from those (hist2D, smktf::probe_sample) for comparison.
// usage: step_hist_main <vol nx ny nz nelts> <u16 0|1> <dmode> <vpos.f32> <out prefix>
//   writes <prefix>.hstep and <prefix>.h2d: the return value (one byte) and the 65536 bytes of hist2DStep() and hist2D();
//          <prefix>.pstep: per probe position 40 floats {return value, inside, cell[3], corners[8][3], hessian_pos[8], value[3]}
//          of probeStep(); <prefix>.phost: the same of smktf::probe_sample on the host's bytes (8-bit data only)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "HipVolumeRenderer.h"
#include "TransferFunctions.h"

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

static void record(std::vector<float> &o, int rc, const smktf::ProbeSample &s) {
  o.push_back((float)rc);
  o.push_back(s.inside ? 1.f : 0.f);
  for (int a = 0; a < 3; ++a) o.push_back((float)s.cell[a]);
  for (int i = 0; i < 8; ++i)
    for (int a = 0; a < 3; ++a) o.push_back(s.corners[i][a]);
  for (int i = 0; i < 8; ++i) o.push_back(s.hessian_pos[i]);
  for (int a = 0; a < 3; ++a) o.push_back(s.value[a]);
}

int main(int argc, char **argv) {
  if (argc != 10) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);
  int a = 1;
  auto vol = slurp(argv[a++]);
  const int nx = atoi(argv[a++]), ny = atoi(argv[a++]), nz = atoi(argv[a++]), ne = atoi(argv[a++]);
  const bool u16 = atoi(argv[a++]) != 0;
  gluvv.dmode = (gluvvDataMode)atoi(argv[a++]);
  auto vp = slurp(argv[a++]);
  const std::string out = argv[a++];
  if (vol.size() != (size_t)nx * ny * nz * ne * (u16 ? 2 : 1) || vp.empty() || vp.size() % 12) {
    fprintf(stderr, "volume or probe positions: size mismatch\n");
    return 2;
  }
  // MetaVolume as the loader leaves it: one brick, largest dimension normalised to 1
  MetaVolume mv;
  Volume v;
  const int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
  mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
  v.currentData = vol.data();
  mv.volumes = &v;
  mv.numSubVols = 1;
  mv.nelts = ne;
  gluvv.mv = &mv;

  HipVolumeRenderer vr(&mv, 0);
  if (!vr.ok()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  vr.useU16(u16 ? 1 : 0);
  if (vr.createVolume(VolRen3DExt, mv.volumes, mv.numSubVols)) return 4;

  std::vector<unsigned char> h(1 + 65536, 0);
  h[0] = (unsigned char)vr.hist2DStep(h.data() + 1);
  if (!spill(out + ".hstep", h.data(), h.size())) return 6;
  std::fill(h.begin(), h.end(), 0);
  h[0] = (unsigned char)vr.hist2D(h.data() + 1);
  if (!spill(out + ".h2d", h.data(), h.size())) return 6;

  const float *pos = (const float *)vp.data();
  std::vector<float> pstep, phost;
  for (size_t i = 0; i < vp.size() / 12; ++i) {
    smktf::ProbeSample s;
    const int rc = vr.probeStep(pos + 3 * i, &s);
    record(pstep, rc, s);
    if (!u16) {
      smktf::ProbeSample t;
      smktf::probe_sample(vol.data(), ne, nx, ny, nz, gluvv.dmode, pos + 3 * i, &t);
      record(phost, 1, t);
    }
  }
  if (!spill(out + ".pstep", pstep.data(), pstep.size() * 4)) return 6;
  if (!u16 && !spill(out + ".phost", phost.data(), phost.size() * 4)) return 6;
  return 0;
}
