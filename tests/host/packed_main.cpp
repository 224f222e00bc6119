// packed_main.cpp -- the host side of the library's statement of the packed voxel and of a region's rows (smk_packed.h), driven
// by lines on stdin; one line of output per line of input.  Numbers are decimal, 32-bit words hexadecimal.
//   pack8 <dtype 0|2> <nelts> <n0> <n1> <n2> <c0> <c1> <c2> <c3>    ->  w0 w1            (n0 < 0: the voxel has no normal)
//   packf <nelts> <n0> <n1> <n2> <c0> <c1> <c2> <c3>                 ->  w0 w1 w2 w3 sep  (channels as words; sep: the word
//                                                                         that belongs into the separate buffer, or "-")
//   unpack8 <dtype 0|2> <nelts> <w0> <w1>                            ->  c0 c1 c2 c3 n0 n1 n2   (a download's values)
//   unpackf <nelts> <w0> <w1> <w2> <w3> <sep or ->                   ->  c0 c1 c2 c3 n0 n1 n2   (channels as words)
//   div <d> <n>                                                      ->  floor(n / d) by step_div / step_divide
//   rows <wide 0|1> <chunk> <g0 x y z> <g1 x y z> <O x y z> <D x y z> ->  upr head tail ox units nvox outside visits
//        every unit of the region's rows, walked in chunks of <chunk> units through step_chunk_origin and step_unit;
//        outside: voxels met outside the stored box; visits: per voxel of the stored box, in address order, how often it was met
//   unit <wide 0|1> <base> <i> <g0 x y z> <g1 x y z> <O x y z> <D x y z> ->  u0 y0 z0 row0 index col q
//        the origin of the chunk that starts at unit <base> and unit <i> of it, for regions too large to walk (the 64-bit
//        division of step_chunk_origin)
// No device, no library: the header's host side only.  tests/test_packed_cpu.py compares it with the tests' own restatements.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../simian-spacemonkey_amd/csrc/smk_packed.h"

static uint32_t normal_word(const int n[3]) { return n[0] < 0 ? SMK_NRM_NONE : smk_nrm_word((uint32_t)n[0], (uint32_t)n[1], (uint32_t)n[2]); }

static void print_unpacked(const uint32_t c[4], uint32_t nw, bool hex) {
  unsigned char g[3];
  smk_nrm_bytes(nw, g);
  printf(hex ? "%08x %08x %08x %08x %u %u %u\n" : "%u %u %u %u %u %u %u\n", c[0], c[1], c[2], c[3], g[0], g[1], g[2]);
}

static void rows(const char *args) {
  int wide, g0[3], g1[3], O[3], D[3];
  unsigned chunk;
  if (sscanf(args, "%d %u %d %d %d %d %d %d %d %d %d %d %d %d", &wide, &chunk, g0, g0 + 1, g0 + 2, g1, g1 + 1, g1 + 2, O, O + 1, O + 2, D, D + 1,
             D + 2) != 14 || !chunk) {
    printf("bad rows line\n");
    return;
  }
  const StepRows R = step_rows(g0, g1, O, D, wide != 0);
  const unsigned long long box_units = R.pitch * (unsigned long long)D[1] * (unsigned long long)D[2];
  std::vector<unsigned char> seen((size_t)D[0] * D[1] * D[2], 0);
  unsigned long long outside = 0;
  auto meet = [&](unsigned long long voxel, bool in_box) {
    if (!in_box || voxel >= seen.size()) ++outside;
    else if (seen[(size_t)voxel] < 9) ++seen[(size_t)voxel];
  };
  for (unsigned long long base = 0; base < R.units; base += chunk) {
    const unsigned lim = R.units - base < chunk ? (unsigned)(R.units - base) : chunk;
    const StepOrigin C = step_chunk_origin(R, base);
    for (unsigned i = 0; i < lim; ++i) {
      unsigned col, q;
      const unsigned long long o = step_unit(R, C, i, col, q);
      const bool in_box = o < box_units && R.ox + col < R.pitch;  // (within the box and within its own stored row)
      if (wide) {
        meet(o, in_box);
      } else {
        if (!step_low_masked(R, col)) meet(2 * o, in_box);
        if (!step_high_masked(R, col)) meet(2 * o + 1, in_box);
      }
    }
  }
  std::string visits(seen.size(), '0');
  for (size_t i = 0; i < seen.size(); ++i) visits[i] = (char)('0' + seen[i]);
  printf("%u %u %u %u %llu %llu %llu %s\n", R.upr, R.head, R.tail, R.ox, R.units, R.nvox, outside, visits.c_str());
}

static void unit(const char *args) {
  int wide, g0[3], g1[3], O[3], D[3];
  unsigned long long base;
  unsigned i, col, q;
  if (sscanf(args, "%d %llu %u %d %d %d %d %d %d %d %d %d %d %d %d", &wide, &base, &i, g0, g0 + 1, g0 + 2, g1, g1 + 1, g1 + 2, O, O + 1, O + 2, D,
             D + 1, D + 2) != 15) {
    printf("bad line\n");
    return;
  }
  const StepRows R = step_rows(g0, g1, O, D, wide != 0);
  const StepOrigin C = step_chunk_origin(R, base);
  const unsigned long long o = step_unit(R, C, i, col, q);
  printf("%u %u %llu %llu %llu %u %u\n", C.u0, C.y0, C.z0, C.row0, o, col, q);
}

int main() {
  std::vector<char> buf(1 << 16);
  while (fgets(buf.data(), (int)buf.size(), stdin)) {
    const char *line = buf.data();
    int dt, nelts, n[3];
    uint32_t c[4], w[4];
    char sep[16];
    unsigned d, num;
    if (sscanf(line, "pack8 %d %d %d %d %d %u %u %u %u", &dt, &nelts, n, n + 1, n + 2, c, c + 1, c + 2, c + 3) == 9) {
      const unsigned char b[4] = {(unsigned char)c[0], (unsigned char)c[1], (unsigned char)c[2], (unsigned char)c[3]};
      const unsigned short h[3] = {(unsigned short)c[0], (unsigned short)c[1], (unsigned short)c[2]};
      const uint2 v = dt == SMK_U8 ? smk_pack_u8(b, nelts, normal_word(n)) : smk_pack_u16(h, nelts, normal_word(n));
      printf("%08x %08x\n", v.x, v.y);
    } else if (sscanf(line, "packf %d %d %d %d %x %x %x %x", &nelts, n, n + 1, n + 2, c, c + 1, c + 2, c + 3) == 8) {
      const int n_in_w = nelts <= 3;
      float f[4];
      memcpy(f, c, sizeof f);
      const uint4 v = smk_pack_f32(f, nelts, normal_word(n), n_in_w);
      printf("%08x %08x %08x %08x ", v.x, v.y, v.z, v.w);
      if (n_in_w || n[0] < 0) printf("-\n");
      else printf("%08x\n", normal_word(n));
    } else if (sscanf(line, "unpack8 %d %d %x %x", &dt, &nelts, w, w + 1) == 4) {
      uint32_t o[4] = {0, 0, 0, 0};
      if (dt == SMK_U8) {
        for (int e = 0; e < nelts; ++e) o[e] = smk_u8_ch(w[0], e);
      } else {
        o[0] = smk_vox8_c0<SMK_U16>(w[0]);
        if (nelts > 1) o[1] = smk_vox8_c1<SMK_U16>(w[0]);
        if (nelts > 2) o[2] = smk_q8_expand(smk_u16_q2(w[1]));
      }
      print_unpacked(o, w[1], false);
    } else if (sscanf(line, "unpackf %d %x %x %x %x %15s", &nelts, w, w + 1, w + 2, w + 3, sep) == 6) {
      uint32_t o[4] = {w[0], nelts > 1 ? w[1] : 0, nelts > 2 ? w[2] : 0, nelts > 3 ? w[3] : 0};
      const uint32_t s = strcmp(sep, "-") ? (uint32_t)strtoul(sep, nullptr, 16) : SMK_NRM_NONE;
      print_unpacked(o, smk_f32_nrm_word(make_uint4(w[0], w[1], w[2], w[3]), nelts, s), true);
    } else if (sscanf(line, "div %u %u", &d, &num) == 2) {
      printf("%u\n", step_divide(num, step_div(d)));
    } else if (!strncmp(line, "rows ", 5)) {
      rows(line + 5);
    } else if (!strncmp(line, "unit ", 5)) {
      unit(line + 5);
    } else {
      printf("bad line\n");
    }
  }
  return 0;
}
