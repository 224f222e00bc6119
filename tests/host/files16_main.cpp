// files16_main.cpp -- drives the 16-bit load of simian-spacemonkey_amd/host/VolumeFiles.{h,cpp} for tests/test_u16_cpu.py,
// the way files_main drives the 8-bit one.
//
//   files16_main load16 <file.trex> <timestep> <out.u16> <out.u8>
//       load_trex with keep16: every brick's 16-bit voxels (host byte order) concatenated in brick order into out.u16, and
//       the 8-bit voxels of the same load -- the reference's path, which the option must not change -- into out.u8
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "VolumeFiles.h"

using namespace smkfiles;

static int spit(const char *path, const void *p, size_t n) {
  FILE *f = fopen(path, "wb");
  if (!f) return 1;
  size_t w = fwrite(p, 1, n, f);
  fclose(f);
  return w == n ? 0 : 1;
}

int main(int argc, char **argv) {
  if (argc != 6 || strcmp(argv[1], "load16")) return 2;
  std::string err;
  LoadedVolume lv;
  size_t n = load_trex(argv[2], atoi(argv[3]), &lv, &err, true);
  if (!n) {
    fprintf(stderr, "%s\n", err.c_str());
    return 4;
  }
  std::vector<unsigned short> all16;
  std::vector<unsigned char> all8;
  int points16 = 1;  // every Volume's currentData is its 16-bit brick
  for (size_t i = 0; i < lv.data16.size(); ++i) {
    all16.insert(all16.end(), lv.data16[i].begin(), lv.data16[i].end());
    points16 &= lv.vols[i].currentData == (unsigned char *)lv.data16[i].data();
  }
  for (auto &d : lv.data) all8.insert(all8.end(), d.begin(), d.end());
  printf("bytes=%zu\nbricks=%d\nbricks16=%zu\npoints16=%d\n", n, lv.mv.numSubVols, lv.data16.size(), points16);
  return spit(argv[4], all16.data(), all16.size() * 2) || spit(argv[5], all8.data(), all8.size());
}
