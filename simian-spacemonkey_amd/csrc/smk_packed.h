// smk_packed.h -- the packed voxel and the rows of a context's region, stated once: every kernel that writes or reads the
// packed voxels of a time step outside the ray-marchers' fetches goes through the expressions below, so that all give the
// same bits.  SMK_PK functions run on host and device; step_div and step_rows (a kernel's parameters) are host-only, the
// ray-marchers' smk_decode_u16 device-only.  The host side needs no device and no context (tests/host/packed_main.cpp).
//
// THE PACKED VOXEL.  A voxel is two or four 32-bit words, by the volume's smk_dtype:
//   SMK_U8   uint2 {c0 | c1 << 8 | c2 << 16 | c3 << 24,  n0 | n1 << 8 | n2 << 16}
//   SMK_U16  uint2 {c0 | c1 << 16,  n0 | n1 << 8 | n2 << 16 | q8(c2) << 24}        (1 to 3 channels)
//            channels 0 and 1 whole; channel 2 as its nearest 8-bit unorm q8(c) = (255 c + 32767) / 65535 in the byte the
//            normal leaves free, which reads back as the 16-bit value 257 q
//   SMK_F32  uint4 {c0, c1, c2, n0 | n1 << 8 | n2 << 16}                            (1 to 3 channels: "n_in_w")
//            uint4 {c0, c1, c2, c3}, the normal word in a SEPARATE buffer of one word per voxel (TimeStep::nrm), which
//            exists only when the volume came with normals                          (4 channels)
// A missing channel is 0; a missing normal is (128, 128, 128), the word SMK_NRM_NONE.  Only the low three bytes of a normal
// word are the normal (readers mask them: the u16 word carries q8(c2) above them).
//
// THE STORED BOX.  A context keeps D[0] x D[1] x D[2] voxels from voxel O of the volume, x fastest, voxel (X, Y, Z) of the box
// at index (Z * D[1] + Y) * D[0] + X of TimeStep::vox, and of TimeStep::nrm where that exists.  The box is the context's
// region [g0, g1) plus its halo, cut at the volume.  Rows of 8-byte voxels are made even in x and y (smk_volume_geometry):
// by one more voxel where the volume has one, else by a pad column past the volume that holds zeros and that nobody
// samples.  So D[0] is even for 8-byte voxels and the box is a whole number of 16-byte units: one f32 voxel, or two 8-byte
// voxels.  16 more bytes are allocated behind it, because the gather kernel loads 8-byte voxels in pairs.
//
// THE REGION'S ROWS (StepRows, below).  The region is ny * nz rows, each a run of nx = g1x - g0x voxels that starts
// g0 - O into the box.  A row is read in whole 16-byte units, so the run of an 8-byte layout is widened to even voxel
// offsets: the first unit's low voxel is masked when g0x - Ox is odd (`head`), the last unit's high voxel when the run
// ends on an odd offset (`tail`).  D[0] is even there, so both masked voxels lie inside the row: nothing is read outside
// the stored box.  With ox = g0x - Ox:   upr = nx (f32),  (ox % 2 + nx + 1) / 2 (8-byte);   units = upr * ny * nz.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/smk.h"

#define SMK_PK __host__ __device__ __forceinline__

// ------------------------------------------------------------------------------------------------ words: encode

constexpr uint32_t SMK_NRM_NONE = 0x00808080u;  // the normal word of a voxel without a normal

SMK_PK uint32_t smk_nrm_word(uint32_t n0, uint32_t n1, uint32_t n2) { return n0 | (n1 << 8) | (n2 << 16); }

// a 16-bit channel as the 8-bit unorm nearest to it, and that field as a 16-bit value again
SMK_PK uint32_t smk_q8(uint32_t s) { return (s * 255u + 32767u) / 65535u; }
SMK_PK uint32_t smk_q8_expand(uint32_t q) { return 257u * q; }
// ... and the byte a 16-bit value falls into, floor(255 s / 65535): the histogram's bin of a u16 channel
SMK_PK uint32_t smk_u16_bin(uint32_t s) { return s / 257u; }

SMK_PK uint2 smk_pack_u8(const unsigned char *ch, int nelts, uint32_t nb) {
  uint32_t d = 0;
  for (int e = 0; e < nelts; ++e) d |= (uint32_t)ch[e] << (8 * e);
  return make_uint2(d, nb);
}

SMK_PK uint2 smk_pack_u16(const unsigned short *ch, int nelts, uint32_t nb) {
  uint32_t d = ch[0];
  if (nelts > 1) d |= (uint32_t)ch[1] << 16;
  if (nelts > 2) nb |= smk_q8(ch[2]) << 24;
  return make_uint2(d, nb);
}

// the channels bit for bit (a NaN keeps its payload).  n_in_w: up to three channels, the normal word in .w; else channel 3
// there, and nb belongs into the separate buffer
SMK_PK uint4 smk_pack_f32(const float *ch, int nelts, uint32_t nb, int n_in_w) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = ch[0];
  if (nelts > 1) v.y = ch[1];
  if (nelts > 2) v.z = ch[2];
  if (n_in_w) v.w = __builtin_bit_cast(float, nb);
  else v.w = ch[3];
  return __builtin_bit_cast(uint4, v);
}

// ------------------------------------------------------------------------------------------------ words: decode

// 8-byte voxels {w0, w1}.  Channel e of a u8 voxel; channels 0 and 1 of layout DT (SMK_U8 or SMK_U16) at the width they are
// stored in; the stored 8-bit field of channel 2 of a u16 voxel
SMK_PK uint32_t smk_u8_ch(uint32_t w0, int e) { return (w0 >> (8 * e)) & 0xffu; }
template <int DT> SMK_PK uint32_t smk_vox8_c0(uint32_t w0) { return DT == SMK_U8 ? smk_u8_ch(w0, 0) : w0 & 0xffffu; }
template <int DT> SMK_PK uint32_t smk_vox8_c1(uint32_t w0) { return DT == SMK_U8 ? smk_u8_ch(w0, 1) : w0 >> 16; }
SMK_PK uint32_t smk_u16_q2(uint32_t w1) { return w1 >> 24; }

// the three normal bytes of a normal word: w1 of an 8-byte voxel, .w of an f32 voxel of up to three channels, the separate
// word of a four-channel one
SMK_PK uint32_t smk_nrm_bits(uint32_t w) { return w & 0x00ffffffu; }
SMK_PK void smk_nrm_bytes(uint32_t w, unsigned char *g) {
  g[0] = (unsigned char)w;
  g[1] = (unsigned char)(w >> 8);
  g[2] = (unsigned char)(w >> 16);
}

// the normal word of f32 voxel v of `nelts` channels; sep: its word of the separate buffer, SMK_NRM_NONE where there is none
SMK_PK uint32_t smk_f32_nrm_word(uint4 v, int nelts, uint32_t sep) { return nelts <= 3 ? v.w : sep; }

// bytes of one element of the caller's arrays
SMK_PK constexpr size_t smk_elem_bytes(int dtype) { return dtype == SMK_U8 ? 1 : dtype == SMK_U16 ? 2 : 4; }

// one voxel corner as the ray-marchers interpolate it: 4 channels (raw: u8 as 0..255 floats, u16 as 0..65535 floats -- its
// third channel 0..255 --, f32 as is) + packed normal bits
struct SmkCorner {
  float c0, c1, c2, c3;
  uint32_t nb;
};

// u16 voxels (SMK_U16, smk.h): uint2 {c0 | c1 << 16, n0 | n1 << 8 | n2 << 16 | q8(c2) << 24}.  The normal bits sit where the
// u8 voxel has them (smk_nrm looks at the low three bytes only), the third channel's 8 bits ride in the spare byte
__device__ __forceinline__ void smk_decode_u16(uint2 v, SmkCorner &k) {
  k.c0 = (float)(v.x & 0xffffu);
  k.c1 = (float)(v.x >> 16);
  k.c2 = (float)(v.y >> 24);
  k.c3 = 0.0f;
  k.nb = v.y;
}

// ------------------------------------------------------------------------------------------------ the region's rows

// floor(n / d) of 32-bit numbers by a multiplication and two shifts (Granlund and Montgomery 1994, figure 4.1): exact for
// every n < 2^32 and d >= 1.  A lane finds its row and column with two of these in place of two integer divisions
struct StepDiv {
  unsigned m, sh1, sh2;
};

inline StepDiv step_div(unsigned d) {
  unsigned l = 0;
  while ((1ull << l) < d) ++l;  // ceil(log2 d)
  StepDiv k;
  k.m = (unsigned)((((1ull << l) - d) << 32) / d + 1);
  k.sh1 = l < 1 ? l : 1;
  k.sh2 = l > 1 ? l - 1 : 0;
  return k;
}

SMK_PK unsigned step_divide(unsigned n, const StepDiv k) {
#ifdef __HIP_DEVICE_COMPILE__
  const unsigned t = __umulhi(k.m, n);
#else
  const unsigned t = (unsigned)(((unsigned long long)k.m * n) >> 32);
#endif
  return (t + ((n - t) >> k.sh1)) >> k.sh2;
}

struct StepRows {
  unsigned long long units;    // rows * upr
  unsigned long long nvox;     // voxels of the region
  unsigned upr;                // 16-byte units per row
  unsigned nx, ny;             // voxels per row, rows per z
  unsigned long long pitch;    // units per stored row: D[0], or D[0] / 2
  unsigned D1;                 // stored rows per z
  unsigned ox, oy, oz;         // the first unit's offset in its stored row; g0 - O in y and z
  unsigned head, tail;         // 8-byte layouts: the first unit's low / the last unit's high voxel lies outside the run
  StepDiv by_upr, by_ny;
};

// the rows of region [g0, g1) in the box of D voxels from O; wide: a unit is one (f32) voxel.  An empty region has units == 0
inline StepRows step_rows(const int g0[3], const int g1[3], const int O[3], const int D[3], bool wide) {
  const unsigned nx = (unsigned)(g1[0] - g0[0]), ox = (unsigned)(g0[0] - O[0]);
  const unsigned long long nz = (unsigned long long)(g1[2] - g0[2]);
  StepRows R;
  R.head = wide ? 0 : ox & 1;
  R.tail = wide ? 0 : (ox + nx) & 1;
  R.upr = wide ? nx : (R.head + nx + 1) / 2;
  R.nx = nx;
  R.ny = (unsigned)(g1[1] - g0[1]);
  R.units = (unsigned long long)R.upr * R.ny * nz;
  R.nvox = (unsigned long long)nx * R.ny * nz;
  R.pitch = wide ? (unsigned long long)D[0] : (unsigned long long)D[0] / 2;
  R.D1 = (unsigned)D[1];
  R.ox = wide ? ox : ox / 2;
  R.oy = (unsigned)(g0[1] - O[1]);
  R.oz = (unsigned)(g0[2] - O[2]);
  R.by_upr = step_div(R.units ? R.upr : 1);
  R.by_ny = step_div(R.units ? R.ny : 1);
  return R;
}

// 8-byte layouts: the low / the high voxel of the unit in column `col` of its row lies outside the run
SMK_PK bool step_low_masked(const StepRows &R, unsigned col) { return R.head && col == 0; }
SMK_PK bool step_high_masked(const StepRows &R, unsigned col) { return R.tail && col == R.upr - 1; }

// where a chunk -- a run of consecutive units of the region's rows -- starts: its first unit's column u0, its row row0 of
// all rows, and that row as y0 of slice z0
struct StepOrigin {
  unsigned u0, y0;
  unsigned long long z0, row0;
};

SMK_PK StepOrigin step_chunk_origin(const StepRows &R, unsigned long long base) {
  StepOrigin C;
  if (R.units <= 0xffffffffull) {  // (every step that fits a device but the very largest: no 64-bit division)
    C.row0 = step_divide((unsigned)base, R.by_upr);
    C.z0 = step_divide((unsigned)C.row0, R.by_ny);
  } else {
    C.row0 = base / R.upr;
    C.z0 = C.row0 / R.ny;
  }
  C.u0 = (unsigned)(base - C.row0 * R.upr);
  C.y0 = (unsigned)(C.row0 - C.z0 * R.ny);
  return C;
}

// unit i of the chunk that starts at C: its index into the slot's 16-byte units, its column `col` in its row, and the rows q
// it lies behind the chunk's first.  (u0 + i must fit 32 bits: u0 < upr, i < the chunk's length)
SMK_PK unsigned long long step_unit(const StepRows &R, const StepOrigin &C, unsigned i, unsigned &col, unsigned &q) {
  const unsigned t = C.u0 + i;
  q = step_divide(t, R.by_upr);
  const unsigned ry = C.y0 + q, zq = step_divide(ry, R.by_ny);
  col = t - q * R.upr;
  const unsigned long long z = C.z0 + zq + R.oz, y = (unsigned long long)(ry - zq * R.ny) + R.oy;
  return (z * R.D1 + y) * R.pitch + R.ox + col;
}
