// smk_step_merge_h.hip -- the multi-field step WITH H and blurred normals (fields + G, H, normals of the summed gradient) made
// INSIDE the time-step ring (smk.h: smk_merge_timestep_h, smk_upload_timestep_fields_h_device; DESIGN.md 3b "Merged fields
// with H").
//
// MetaVolume::mergeMV with addG, addH and blurnorms (MetaVolume.cpp:1109-1268; gluvv.cpp's -addH and -blurNormals: the data
// modes V1GH, V2GH) is a host program that runs before the renderer starts.  A step whose fields are new on the device gets here
// what smk_merge_fields_h_device / smk_merge_fields_h_f32_device (and, in a u16 ring, smk_quantize_u16_device) and
// smk_upload_timestep_device would make of them, bit for bit, as two kernels on the caller's stream that write the packed
// voxels of a ring slot: no scratch arrays, no host wait.
//
// H reads the summed gradient S of the six neighbours and a blurred normal that of the 26, each a central difference of every
// field: the stencil reaches 2 voxels, which smk_step_merge.hip's register march (reach 1) does not hold.  Both kernels here
// work on tiles of MH_TX x MH_TY x MH_TZ voxels of the stored box, as smk_step_derive.hip's do:
//   F  the fields of the tile with a 2-voxel apron, one 32-bit word per voxel: the channel word of an 8-byte voxel (all fields
//      of a u8 or u16 ring at once), or ONE float field of an f32 ring, which then takes a turn per field;
//   S  the summed gradient (three floats, one plane each) of the tile with a 1-voxel apron, made from F: 0 on the volume's
//      border and outside it, merge_grad_add once per field, fields ascending.
// 20 736 + 40 800 bytes of LDS: two workgroups fit a CU.  Tile rows start on even x, so two 8-byte voxels load as one 16-byte unit.
//   pass 1 (smk_k_merge_h_stats): |S| and, with add_h, hs of every interior voxel -> {max magnitude, min H, max H}, ordered-int
//          atomics per wave into the OUTPUT slot's words (TimeStep::pass1_words), which a one-wave kernel seeded on the stream;
//          a capped grid strides over the tiles;
//   pass 2 (smk_k_merge_h_write): S again, G, H and the normal, and one 8- or 16-byte store of the packed voxel (and the
//          normal word of a four-channel f32 voxel).
// The arithmetic is smk_prep.hip's, through smk_prep_device.h; the packed voxel is smk_packed.h's.
// Instances of the two kernels over parameter types of their own serve sharded contexts (MergeHShardParams: a packed step of
// the ring; smk_step_extremes_h_device, smk_merge_timestep_h_shard) and a decomposed simulation's own dense blocks of the
// volume (MergeHBlockParams: smk_block_extremes_h_device, smk_upload_timestep_fields_h_block_device).
#include <limits.h>

#include <algorithm>

#include "smk_step_stencil.h"

namespace {

constexpr int MH_TX = 32, MH_TY = 8, MH_TZ = 8;
constexpr int MH_FX = MH_TX + 4, MH_FY = MH_TY + 4, MH_FZ = MH_TZ + 4, MH_FN = MH_FX * MH_FY * MH_FZ;  // 5184 words
constexpr int MH_SX = MH_TX + 2, MH_SY = MH_TY + 2, MH_SZ = MH_TZ + 2, MH_SN = MH_SX * MH_SY * MH_SZ;  // 3400 floats, three times
constexpr int MH_FSY = MH_FX, MH_FSZ = MH_FX * MH_FY, MH_SSY = MH_SX, MH_SSZ = MH_SX * MH_SY;
static_assert(MH_TX * MH_TY == 256 && MH_TX % 2 == 0, "a thread per (x, y) of the tile; tile rows start on even x");
static_assert((MH_FN + 3 * MH_SN) * 4 <= 64 * 1024, "two workgroups per CU");
constexpr unsigned MH_STATS_BLOCKS = 2048;  // pass 1's grid: 8 workgroups for each of 256 CUs (its atomics land on one cache line)

struct MergeHParams {
  const void *src;    // the source slot's packed voxels [D2][D1][D0] ...
  const void *f[3];   // ... or the dense fields [N2][N1][N0], one array each
  void *out;          // the output slot's packed voxels
  uint32_t *nrm;      // its separate normal words (four-channel f32 with normals), else null
  int *w;             // the output slot's words {max magnitude, min H, max H}, ordered-int
  int N[3], D[3];     // the volume; the stored box (origin 0), D >= N with a pad column or row of 8-byte voxels.  The kernels rely
                      // on D[2] == N[2], on D == N for f32 voxels and on an even D[0] otherwise: smk_step_stencil_refusals checks
  int add_h, compat, blur, normals;
  int gx, gy, ntiles;  // tiles per row of tiles, rows of tiles per slice of tiles, tiles in all
};

// The SHARD instances (smk.h: smk_step_extremes_h_device, smk_merge_timestep_h_shard): the stored box lies anywhere in the
// volume.  Tiles, the aprons of F and S and every index into the slots stay LOCAL to the stored box, so a 16-byte unit of two
// 8-byte voxels starts on an even local x whatever the parity of O[0]; the border of the volume, its pad and the normals'
// border are decided on GLOBAL voxels O + local.  F is 0 outside the stored box, so S, H and the normals within 2 voxels of a
// face of the box that is no face of the volume are made from voxels this context does not hold: pass 2 writes zeros (normal
// 128) outside the valid box.  Pass 1 takes the region's voxels alone and leaves its extremes in the caller's eight words, min
// H complemented; pass 2 reads the combined words.  A parameter TYPE of its own: the unsharded instances' code is what it was.
struct MergeHShardParams : MergeHParams {
  SmkShardBox B;
  int *words_out;       // pass 1: the export
  const int *words_in;  // pass 2: the combined extremes
};
// The BLOCK instances (smk.h: smk_block_extremes_h_device, smk_upload_timestep_fields_h_block_device): shard instances whose
// fields are a rank's own dense blocks of the volume, all laid out by one smk_block that lies anywhere.  Only the SOURCE
// differs: a voxel is read when it lies inside C = block ∩ stored box ∩ volume, at (local - bo) through the block's pitches,
// (StencilBlockSrc: bo, c0, c1, py, pz), and F is 0 outside C.  Again a parameter type of its own
struct MergeHBlockParams : MergeHShardParams, StencilBlockSrc {};

// the volume's 1-voxel border (and everything outside the volume) at local voxel (X, Y, Z)
template <class PT>
__device__ __forceinline__ bool mh_border(const PT &P, int X, int Y, int Z) {
  return is_border(P.N[0], P.N[1], P.N[2], stencil_glob(P, 2, Z), stencil_glob(P, 1, Y), stencil_glob(P, 0, X));
}

// the turns F takes: one per field of an f32 ring, one for all fields of an 8-byte voxel
constexpr int mh_turns(int SRC, int NF) { return stencil_ring(SRC) == SMK_F32 ? NF : 1; }

// field e of a word of F as the float the gradient is taken of: (float)v of an integer, unscaled
template <int SRC>
__device__ __forceinline__ float mh_val(uint32_t w, int e) {
  constexpr int RING = stencil_ring(SRC);
  if (RING == SMK_F32) return __uint_as_float(w);
  if (RING == SMK_U8) return (float)smk_u8_ch(w, e);
  return (float)(e ? smk_vox8_c1<SMK_U16>(w) : smk_vox8_c0<SMK_U16>(w));
}

// F of the tile at (x0, y0, z0) for turn p; what lies outside the volume is 0 and is never used.  (On a shard, what the
// source does not hold is 0 too, and is used by the voxels of the rim alone)
template <int SRC, int NF, class PT>
__device__ __forceinline__ void mh_load(const PT &P, int x0, int y0, int z0, int p, uint32_t *F) {
  constexpr int RING = stencil_ring(SRC);
  if (SRC == SRC_PK_U8 || SRC == SRC_PK_U16) {  // two voxels per 16-byte unit (x0 - 2 is even, and so is D[0]): their channel words are .x and .z
    constexpr int UPR = MH_FX / 2;
    for (int u = threadIdx.x; u < UPR * MH_FY * MH_FZ; u += 256) {
      const int cu = u % UPR, row = u / UPR, ly = row % MH_FY, lz = row / MH_FY;
      const int X = x0 - 2 + 2 * cu, Y = y0 - 2 + ly, Z = z0 - 2 + lz;
      uint32_t a = 0u, b = 0u;
      // (the unsharded test spelled out here: through stencil_held the compiler lays these instances' branches out differently)
      if (stencil_shard<PT> ? stencil_held(P, X, Y, Z) : (X >= 0 && X < P.N[0] && Y >= 0 && Y < P.N[1] && Z >= 0 && Z < P.N[2])) {
        const uint4 v = ((const uint4 *)P.src)[(((size_t)Z * P.D[1] + Y) * P.D[0] + X) >> 1];
        a = v.x;
        if (stencil_shard<PT> ? stencil_glob(P, 0, X) + 1 < P.N[0] : X + 1 < P.N[0]) b = v.z;
      }
      F[row * MH_FX + 2 * cu] = a;
      F[row * MH_FX + 2 * cu + 1] = b;
    }
  } else {
    for (int t = threadIdx.x; t < MH_FN; t += 256) {
      const int lx = t % MH_FX, row = t / MH_FX, ly = row % MH_FY, lz = row / MH_FY;
      const int X = x0 - 2 + lx, Y = y0 - 2 + ly, Z = z0 - 2 + lz;
      uint32_t a = 0u;
      if (stencil_held(P, X, Y, Z)) {
        if (SRC == SRC_PK_F32) {
          const uint4 v = ((const uint4 *)P.src)[((size_t)Z * P.D[1] + Y) * P.D[0] + X];
          a = p == 0 ? v.x : p == 1 ? v.y : v.z;
        } else {
          size_t o;
          if constexpr (stencil_block<PT>) o = (size_t)(Z - P.bo[2]) * (size_t)P.pz + (size_t)(Y - P.bo[1]) * (size_t)P.py + (size_t)(X - P.bo[0]);
          else o = ((size_t)Z * P.N[1] + Y) * P.N[0] + X;
          if (RING == SMK_F32) {
            a = ((const uint32_t *)P.f[p])[o];
          } else {  // the channel word an 8-byte voxel would hold
#pragma unroll
            for (int e = 0; e < NF; ++e)
              a |= RING == SMK_U8 ? (uint32_t)((const unsigned char *)P.f[e])[o] << (8 * e) : (uint32_t)((const unsigned short *)P.f[e])[o] << (16 * e);
          }
        }
      }
      F[t] = a;
    }
  }
}

// S of the tile with its 1-voxel apron, and own[p][tz]: the words of this thread's voxels (their fields, as stored).  Every
// thread of the workgroup calls this; S is whole behind it
template <int SRC, int NF, class PT>
__device__ __forceinline__ void mh_tile(const PT &P, int x0, int y0, int z0, uint32_t *F, float *S, uint32_t own[][MH_TZ]) {
  constexpr int TURNS = mh_turns(SRC, NF);
  const int tx = threadIdx.x % MH_TX, ty = threadIdx.x / MH_TX;
#pragma unroll
  for (int p = 0; p < TURNS; ++p) {
    mh_load<SRC, NF>(P, x0, y0, z0, p, F);
    __syncthreads();
#pragma unroll
    for (int tz = 0; tz < MH_TZ; ++tz) own[p][tz] = F[(tz + 2) * MH_FSZ + (ty + 2) * MH_FSY + tx + 2];
    for (int t = threadIdx.x; t < MH_SN; t += 256) {
      const int lx = t % MH_SX, row = t / MH_SX, ly = row % MH_SY, lz = row / MH_SY;
      const int X = x0 - 1 + lx, Y = y0 - 1 + ly, Z = z0 - 1 + lz;
      float g[3];
      if (p == 0) merge_grad_zero(g);
      else g[0] = S[t], g[1] = S[MH_SN + t], g[2] = S[2 * MH_SN + t];
      if (!mh_border(P, X, Y, Z)) {  // (the border, and everything outside the volume, stays 0)
        const int l = (lz + 1) * MH_FSZ + (ly + 1) * MH_FSY + lx + 1;
#pragma unroll
        for (int e = 0; e < (TURNS == 1 ? NF : 1); ++e) {
          const int fe = TURNS == 1 ? e : p;
          merge_grad_add(g, mh_val<SRC>(F[l + 1], fe), mh_val<SRC>(F[l - 1], fe), mh_val<SRC>(F[l + MH_FSY], fe), mh_val<SRC>(F[l - MH_FSY], fe),
                         mh_val<SRC>(F[l + MH_FSZ], fe), mh_val<SRC>(F[l - MH_FSZ], fe));
        }
      }
      S[t] = g[0], S[MH_SN + t] = g[1], S[2 * MH_SN + t] = g[2];
    }
    __syncthreads();  // (the next turn overwrites F; S is read behind the last)
  }
}

__device__ __forceinline__ void mh_s(const float *S, int l, float g[3]) { g[0] = S[l], g[1] = S[MH_SN + l], g[2] = S[2 * MH_SN + l]; }

// hs of the INTERIOR voxel at index l of S whose summed gradient is g (the neighbours on the border hold 0)
__device__ __forceinline__ float mh_hs(const float *S, int l, const float g[3], int compat) {
  float xp[3], xm[3], yp[3], ym[3], zp[3], zm[3], gm, hs;
  mh_s(S, l + 1, xp);
  mh_s(S, l - 1, xm);
  mh_s(S, l + MH_SSY, yp);
  mh_s(S, l - MH_SSY, ym);
  mh_s(S, l + MH_SSZ, zp);
  mh_s(S, l - MH_SSZ, zm);
  gh_from_grads(g, xp, xm, yp, ym, zp, zm, compat, gm, hs);
  return hs;
}

__global__ __launch_bounds__(64) void smk_k_merge_h_seed_words(int *w) {
  if (threadIdx.x < 3) w[threadIdx.x] = threadIdx.x == 0 ? MERGE_MAX_SEED : threadIdx.x == 1 ? ORD_POS_INF : ORD_NEG_INF;
}

// the eight words of an export (smk.h, smk_step_extremes_h_device): the maximum, min H complemented so that all combine by
// maximum, max H, then five unused words
__global__ __launch_bounds__(64) void smk_k_merge_h_seed_export(int *w) {
  if (threadIdx.x < 8) w[threadIdx.x] = threadIdx.x == 0 ? MERGE_MAX_SEED : threadIdx.x == 1 ? ~ORD_POS_INF : threadIdx.x == 2 ? ORD_NEG_INF : INT_MIN;
}

template <int SRC, int NF, class PT = MergeHParams>
__global__ __launch_bounds__(256) void smk_k_merge_h_stats(const PT P) {
  __shared__ uint32_t F[MH_FN];
  __shared__ float S[3 * MH_SN];
  static_assert(sizeof(uint32_t) * MH_FN + sizeof(float) * 3 * MH_SN == 61536, "the shard and block instances add nothing to the LDS: two workgroups per CU");
  constexpr bool FLT = stencil_ring(SRC) != SMK_U8;  // (a u16 ring's G and H are the float entry's)
  const int tx = threadIdx.x % MH_TX, ty = threadIdx.x / MH_TX;
  int m = MERGE_MAX_SEED, hmin = ORD_POS_INF, hmax = ORD_NEG_INF;
  for (int tile = blockIdx.x; tile < P.ntiles; tile += gridDim.x) {
    const int bx = tile % P.gx, by = (tile / P.gx) % P.gy, bz = tile / (P.gx * P.gy);
    const int x0 = bx * MH_TX, y0 = by * MH_TY, z0 = bz * MH_TZ;
    if constexpr (stencil_shard<PT>) {  // a tile of halo voxels alone has nothing to add (the whole workgroup skips it)
      if (x0 >= P.B.r1[0] || x0 + MH_TX <= P.B.r0[0] || y0 >= P.B.r1[1] || y0 + MH_TY <= P.B.r0[1] || z0 >= P.B.r1[2] || z0 + MH_TZ <= P.B.r0[2])
        continue;
    }
    uint32_t own[mh_turns(SRC, NF)][MH_TZ];
    mh_tile<SRC, NF>(P, x0, y0, z0, F, S, own);
    const int X = x0 + tx, Y = y0 + ty;
    bool mine = true;
    if constexpr (stencil_shard<PT>) mine = X >= P.B.r0[0] && X < P.B.r1[0] && Y >= P.B.r0[1] && Y < P.B.r1[1];  // the region's voxels alone
    for (int tz = 0; tz < MH_TZ; ++tz) {
      const int Z = z0 + tz;
      if constexpr (stencil_shard<PT>) {
        if (!mine || Z < P.B.r0[2] || Z >= P.B.r1[2]) continue;
      }
      if (mh_border(P, X, Y, Z)) continue;  // (and everything outside the volume)
      const int l = (tz + 1) * MH_SSZ + (ty + 1) * MH_SSY + tx + 1;
      float g[3];
      mh_s(S, l, g);
      const float mag = merge_mag(g);
      m = FLT ? merge_max_take_f32(m, mag) : merge_max_take(m, mag);
      if (P.add_h) {
        const float hs = mh_hs(S, l, g, P.compat);
        if (merge_h_counts(FLT, hs)) {
          hmin = min(hmin, f2o(hs));
          hmax = max(hmax, f2o(hs));
        }
      }
    }
    // (the next tile writes S behind its first barrier, which every thread reaches behind these reads)
  }
  m = wave_max(m);
  hmin = wave_min(hmin);
  hmax = wave_max(hmax);
  if ((threadIdx.x & 63) == 0) {
    if constexpr (stencil_shard<PT>) {
      atomicMax(&P.words_out[0], m);
      if (P.add_h) {
        atomicMax(&P.words_out[1], ~hmin);
        atomicMax(&P.words_out[2], hmax);
      }
    } else {
      atomicMax(&P.w[0], m);
      if (P.add_h) {
        atomicMin(&P.w[1], hmin);
        atomicMax(&P.w[2], hmax);
      }
    }
  }
}

template <int SRC, int NF, class PT = MergeHParams>
__global__ __launch_bounds__(256) void smk_k_merge_h_write(const PT P) {
  __shared__ uint32_t F[MH_FN];
  __shared__ float S[3 * MH_SN];
  constexpr int RING = stencil_ring(SRC), TURNS = mh_turns(SRC, NF);
  const int x0 = blockIdx.x * MH_TX, y0 = blockIdx.y * MH_TY, z0 = blockIdx.z * MH_TZ;
  uint32_t own[TURNS][MH_TZ];
  mh_tile<SRC, NF>(P, x0, y0, z0, F, S, own);
  float maxm, hmin, hmax;  // (a shard's come combined from the caller's words, min H complemented)
  if constexpr (stencil_shard<PT>) {
    maxm = o2f(P.words_in[0]);
    merge_h_extremes(~P.words_in[1], P.words_in[2], hmin, hmax);
  } else {
    maxm = o2f(P.w[0]);
    merge_h_extremes(P.w[1], P.w[2], hmin, hmax);
  }
  const int tx = threadIdx.x % MH_TX, ty = threadIdx.x / MH_TX, X = x0 + tx, Y = y0 + ty;
  if (X >= P.D[0] || Y >= P.D[1]) return;
  const int GX = stencil_glob(P, 0, X), GY = stencil_glob(P, 1, Y);
  const int ne = NF + 1 + P.add_h;
#pragma unroll
  for (int tz = 0; tz < MH_TZ; ++tz) {
    const int Z = z0 + tz, GZ = stencil_glob(P, 2, Z);
    if (Z >= P.D[2]) break;
    const size_t o = ((size_t)Z * P.D[1] + Y) * P.D[0] + X;
    if (GX >= P.N[0] || GY >= P.N[1]) {  // the pad column or row of an 8-byte box: zeros, as after an upload
      ((uint2 *)P.out)[o] = make_uint2(0u, 0u);
      continue;
    }
    if constexpr (stencil_shard<PT>) {  // the rim: zeros that carry no normal (a four-channel f32 voxel's goes to the separate buffer)
      if (X < P.B.v0[0] || X >= P.B.v1[0] || Y < P.B.v0[1] || Y >= P.B.v1[1] || Z < P.B.v0[2] || Z >= P.B.v1[2]) {
        if (RING != SMK_F32) {
          ((uint2 *)P.out)[o] = make_uint2(0u, SMK_NRM_NONE);
        } else {
          ((uint4 *)P.out)[o] = make_uint4(0u, 0u, 0u, ne <= 3 ? SMK_NRM_NONE : 0u);
          if (ne == 4 && P.nrm) P.nrm[o] = SMK_NRM_NONE;
        }
        continue;
      }
    }
    const int l = (tz + 1) * MH_SSZ + (ty + 1) * MH_SSY + tx + 1;
    float g[3];
    mh_s(S, l, g);
    const float mag = merge_mag(g);
    float hs = 0.f;  // (the border's)
    if (P.add_h && !is_border(P.N[0], P.N[1], P.N[2], GZ, GY, GX)) hs = mh_hs(S, l, g, P.compat);
    uint32_t nw = SMK_NRM_NONE;
    if (P.normals) {
      float gn[3];
      unsigned char n[3];
      // (Z, Y, X) -> index of S: l moved by the offset; only interior voxels are asked for, all inside the apron
      nrm_gradient(P.blur, P.N[0], P.N[1], P.N[2], GZ, GY, GX, gn,
                   [&](int si, int sj, int sk, float s[3]) { mh_s(S, l + (si - GZ) * MH_SSZ + (sj - GY) * MH_SSY + (sk - GX), s); });
      if (RING == SMK_U8) nrm_store(gn, n);
      else nrm_store_f32(gn, n);  // (u16: the float entry's normals, made from the floats before any quantisation)
      nw = smk_nrm_word(n[0], n[1], n[2]);
    }
    if (RING == SMK_U8) {  // (the fields are copied, on the border too)
      unsigned char q[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < NF; ++e) q[e] = (unsigned char)smk_u8_ch(own[0][tz], e);
      q[NF] = merge_gmag_u8(mag, maxm);
      if (P.add_h) q[(NF + 1) & 3] = merge_h_u8(hs, hmin, hmax);
      ((uint2 *)P.out)[o] = smk_pack_u8(q, ne, nw);
    } else if (RING == SMK_U16) {
      unsigned short s[4] = {0, 0, 0, 0};
      s[0] = (unsigned short)smk_vox8_c0<SMK_U16>(own[0][tz]);
      if (NF > 1) s[1] = (unsigned short)smk_vox8_c1<SMK_U16>(own[0][tz]);
      s[NF] = quant_u16(merge_g_f32(mag, maxm));  // smk_quantize_u16_device of the float G, and of the float H
      if (P.add_h) s[(NF + 1) & 3] = quant_u16(merge_h_f32(hs, hmin, hmax));
      ((uint2 *)P.out)[o] = smk_pack_u16(s, ne, nw);
    } else {
      float f[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int e = 0; e < NF; ++e) f[e] = __uint_as_float(own[e % TURNS][tz]);  // raw words: NaN payloads and -0 travel
      f[NF] = merge_g_f32(mag, maxm);
      if (P.add_h) f[(NF + 1) & 3] = merge_h_f32(hs, hmin, hmax);
      ((uint4 *)P.out)[o] = smk_pack_f32(f, ne, nw, ne <= 3);
      if (ne == 4 && P.nrm) P.nrm[o] = nw;
    }
  }
}

// The seed and pass 1 (PASS_1: into the slot's words, a shard's and a block's into the caller's words), pass 2, or both, of the
// instance that reads the ring's type -- a packed step of the ring (PACKED) or dense fields -- with the series' fields
template <bool PACKED, class PT>
hipError_t launch_merge_h(const smk_ctx *c, const PT &P, int passes, hipStream_t s) {
  return stencil_dispatch<PACKED>(c->dtype, c->nelts - 1 - P.add_h, [&](auto src, auto nf) {
    constexpr int SRC = decltype(src)::value, NF = decltype(nf)::value;
    if (passes & PASS_1) {
      if constexpr (stencil_shard<PT>) hipLaunchKernelGGL(smk_k_merge_h_seed_export, dim3(1), dim3(64), 0, s, P.words_out);
      else hipLaunchKernelGGL(smk_k_merge_h_seed_words, dim3(1), dim3(64), 0, s, P.w);
      hipLaunchKernelGGL((smk_k_merge_h_stats<SRC, NF, PT>), dim3(std::min<unsigned>((unsigned)P.ntiles, MH_STATS_BLOCKS)), dim3(256), 0, s, P);
    }
    if (passes & PASS_2) {
      const dim3 grid((unsigned)P.gx, (unsigned)P.gy, (unsigned)(P.ntiles / (P.gx * P.gy)));
      hipLaunchKernelGGL((smk_k_merge_h_write<SRC, NF, PT>), grid, dim3(256), 0, s, P);
    }
    return hipGetLastError();
  });
}

// what both entries refuse before they look at their data (smk_step_stencil_refusals); add_h is 0 or 1
StencilEntry merge_h_entry(const smk_ctx *c, const char *who, int add_h) {
  char nelts_why[160] = "";
  const int top = c->dtype == SMK_U16 ? 3 : 4;
  if (add_h && c->dtype == SMK_U16 && c->nelts != 3)
    snprintf(nelts_why, sizeof nelts_why, "add_h on a 16-bit ring of nelts %d: a u16 voxel holds three channels, one field, G and H (nelts 3)", c->nelts);
  else if (c->nelts - 1 - add_h < 1)
    snprintf(nelts_why, sizeof nelts_why, "the series has nelts %d: with add_h %d a multi-field step is at least one field, G%s (nelts >= %d)", c->nelts,
             add_h, add_h ? " and H" : "", 2 + add_h);
  else if (c->nelts > top) snprintf(nelts_why, sizeof nelts_why, "internal: nelts %d of a voxel type that holds %d channels", c->nelts, top);
  return {who,
          "the stencil reaches 2 voxels beyond region + halo, and G and H are scaled by the whole volume's three extremes (maximum magnitude, "
          "min H, max H); the two-call forms are smk_step_extremes_h_device + smk_merge_timestep_h_shard and, from blocks, "
          "smk_block_extremes_h_device + smk_upload_timestep_fields_h_block_device",
          nelts_why, "smk_merge_fields_h_device"};
}

// the flags both entries take: 0 or 1
int merge_h_flags(smk_ctx *c, const char *who, int add_h, int blur) {
  if (add_h != 0 && add_h != 1) FAIL(c, "%s: add_h %d is neither 0 nor 1", who, add_h);
  if (blur != 0 && blur != 1) FAIL(c, "%s: blur %d is neither 0 nor 1", who, blur);
  return 0;
}

// What every instance takes of the context: the volume, the stored box, its tiles, the flags, and with `fields` the series'
// dense fields; no packed source and no output yet.  More tiles than a grid holds (2^42 voxels, or 2^19 rows or slices: no ring
// holds such a step) are refused in the words of the entries of the whole volume (`whole`), or of the shard and block entries
int merge_h_common(smk_ctx *c, const char *who, bool whole, const void *const *fields, int add_h, int compat, int blur, MergeHParams &P) {
  const long long gx = (c->D[0] + MH_TX - 1) / MH_TX, gy = (c->D[1] + MH_TY - 1) / MH_TY, gz = (c->D[2] + MH_TZ - 1) / MH_TZ;
  if (gx * gy * gz > 0x7fffffffLL || gy > 65535 || gz > 65535) {
    if (whole) FAIL(c, "%s: a %dx%dx%d volume has more tiles than a grid holds", who, c->N[0], c->N[1], c->N[2]);
    FAIL(c, "%s: a %dx%dx%d stored box has more tiles than a grid holds", who, c->D[0], c->D[1], c->D[2]);
  }
  P.src = nullptr;
  for (int e = 0; e < 3; ++e) P.f[e] = fields && e < c->nelts - 1 - add_h ? fields[e] : nullptr;
  P.out = nullptr;
  P.nrm = nullptr;
  P.w = nullptr;
  for (int a = 0; a < 3; ++a) {
    P.N[a] = c->N[a];
    P.D[a] = c->D[a];
  }
  P.add_h = add_h;
  P.compat = compat ? 1 : 0;
  P.blur = blur;
  P.normals = c->have_normals ? 1 : 0;
  P.gx = (int)gx;
  P.gy = (int)gy;
  P.ntiles = (int)(gx * gy * gz);
  return 0;
}

// the two passes inside the producer frame; ksrc: the source slot, or -1 (dense fields)
int merge_h_enqueue(smk_ctx *c, const char *who, const void *const *fields, int ksrc, int step_out, int add_h, int compat, int blur, hipStream_t s) {
  MergeHParams P;
  if (merge_h_common(c, who, true, fields, add_h, compat, blur, P)) return 1;
  return smk_step_produce(c, who, step_out, ksrc, -1, s, [&](TimeStep &T, const TimeStep *S, const TimeStep *) -> int {
    P.src = S ? S->vox : nullptr;
    P.out = T.vox;
    P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
    P.w = T.pass1_words;
    HIPCHK(c, S ? launch_merge_h<true>(c, P, PASS_1 | PASS_2, s) : launch_merge_h<false>(c, P, PASS_1 | PASS_2, s));
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------- the shard entries

constexpr int MH_REACH = 2;  // H reads S of the six neighbours, a blurred normal that of the 26, and S the fields' of theirs: the apron of F

StencilEntry merge_h_shard_entry(const smk_ctx *c, const char *who, int add_h) {
  StencilEntry E = merge_h_entry(c, who, add_h);
  E.sharded_why = "";
  return E;
}

// the shard's parameters without the source's: the export finds its slot before the frame, the write pass inside it
int merge_h_shard_params(smk_ctx *c, const char *who, int add_h, int compat, int blur, MergeHShardParams &P) {
  if (merge_h_common(c, who, false, nullptr, add_h, compat, blur, P)) return 1;
  P.words_out = nullptr;
  P.words_in = nullptr;
  return 0;
}

// ---------------------------------------------------------------------------------------------- the block entries

// What both block entries refuse, and the shard's parameters with the block's fields as the source (B: the region, and C shrunk
// by the reach as the result's valid box).  step_out: null for the export
int merge_h_block_params(smk_ctx *c, const char *who, const int *step_out, const void *const *d_fields, int nf, smk_dtype dt, const smk_block *b,
                         int add_h, int compat, int blur, SmkBlockView &V, MergeHBlockParams &P) {
  if (merge_h_flags(c, who, add_h, blur)) return 1;
  if (smk_step_block_refusals(c, merge_h_shard_entry(c, who, add_h), MH_REACH, step_out, b, V)) return 1;
  if (stencil_fields_refusals(c, who, d_fields, nf, dt, &add_h, -1, nullptr)) return 1;
  if (merge_h_common(c, who, false, d_fields, add_h, compat, blur, P)) return 1;
  stencil_block_src(c, b, V, P);
  smk_step_block_box(c, V, MH_REACH, P.B);
  P.words_out = nullptr;
  P.words_in = nullptr;
  return 0;
}

}  // namespace

extern "C" int smk_step_extremes_h_device(smk_ctx *c, int step_src, int add_h, int compat, void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_step_extremes_h_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (merge_h_flags(c, who, add_h, 0) || stencil_words_refusals(c, who, d_words)) return 1;
  int ksrc = -1;
  if (smk_step_shard_refusals(c, merge_h_shard_entry(c, who, add_h), MH_REACH, step_src, nullptr, &ksrc)) return 1;
  MergeHShardParams P;
  if (merge_h_shard_params(c, who, add_h, compat, 0, P)) return 1;
  const TimeStep &S = c->ts[(size_t)ksrc];
  P.src = S.vox;
  smk_step_shard_box(c, S, MH_REACH, P.B);
  P.words_out = (int *)d_words;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_read(c, ksrc, -1, s, [&]() -> int {
    HIPCHK(c, launch_merge_h<true>(c, P, PASS_1, s));
    return 0;
  });
}

extern "C" int smk_merge_timestep_h_shard(smk_ctx *c, int step_src, int step_out, int add_h, int compat, int blur, const void *d_words,
                                          void *stream) {
  if (!c) return 1;
  const char *who = "smk_merge_timestep_h_shard";
  HIPCHK(c, hipSetDevice(c->device));
  if (merge_h_flags(c, who, add_h, blur)) return 1;
  int ksrc = -1;
  if (smk_step_shard_refusals(c, merge_h_shard_entry(c, who, add_h), MH_REACH, step_src, &step_out, &ksrc)) return 1;
  MergeHShardParams P;
  if (stencil_words_refusals(c, who, d_words) || merge_h_shard_params(c, who, add_h, compat, blur, P)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, step_out, ksrc, -1, s, [&](TimeStep &T, const TimeStep *S, const TimeStep *) -> int {
    P.src = S->vox;
    P.out = T.vox;
    P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
    smk_step_shard_box(c, *S, MH_REACH, P.B);
    P.words_in = (const int *)d_words;
    HIPCHK(c, launch_merge_h<true>(c, P, PASS_2, s));
    smk_step_shard_done(c, *S, MH_REACH, P.B, T);
    return 0;
  });
}

extern "C" int smk_block_extremes_h_device(smk_ctx *c, const void *const *d_fields, int nf, smk_dtype dtype, const smk_block *b, int add_h,
                                           int compat, void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_block_extremes_h_device";
  HIPCHK(c, hipSetDevice(c->device));
  SmkBlockView V;
  MergeHBlockParams P;
  if (stencil_words_refusals(c, who, d_words) || merge_h_block_params(c, who, nullptr, d_fields, nf, dtype, b, add_h, compat, 0, V, P)) return 1;
  P.words_out = (int *)d_words;
  HIPCHK(c, launch_merge_h<false>(c, P, PASS_1, stream ? (hipStream_t)stream : c->stream));
  return 0;
}

extern "C" int smk_upload_timestep_fields_h_block_device(smk_ctx *c, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                                         const smk_block *b, int add_h, int compat, int blur, const void *d_words,
                                                         void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_fields_h_block_device";
  HIPCHK(c, hipSetDevice(c->device));
  SmkBlockView V;
  MergeHBlockParams P;
  if (merge_h_block_params(c, who, &timestep, d_fields, nf, field_dtype, b, add_h, compat, blur, V, P) || stencil_words_refusals(c, who, d_words))
    return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, timestep, -1, -1, s, [&](TimeStep &T, const TimeStep *, const TimeStep *) -> int {
    P.out = T.vox;
    P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
    P.words_in = (const int *)d_words;
    HIPCHK(c, launch_merge_h<false>(c, P, PASS_2, s));
    smk_step_block_done(c, V, MH_REACH, P.B, T);
    return 0;
  });
}

extern "C" int smk_merge_timestep_h(smk_ctx *c, int step_src, int step_out, int add_h, int compat, int blur, void *stream) {
  if (!c) return 1;
  const char *who = "smk_merge_timestep_h";
  HIPCHK(c, hipSetDevice(c->device));
  if (merge_h_flags(c, who, add_h, blur)) return 1;
  int ksrc = -1;
  if (smk_step_stencil_refusals(c, merge_h_entry(c, who, add_h), step_out, &step_src, &ksrc)) return 1;
  return merge_h_enqueue(c, who, nullptr, ksrc, step_out, add_h, compat, blur, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_upload_timestep_fields_h_device(smk_ctx *c, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype, int sx,
                                                   int sy, int sz, int add_h, int compat, int blur, void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_fields_h_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (merge_h_flags(c, who, add_h, blur)) return 1;
  if (smk_step_stencil_refusals(c, merge_h_entry(c, who, add_h), timestep, nullptr, nullptr)) return 1;
  const int sizes[3] = {sx, sy, sz};
  if (stencil_fields_refusals(c, who, d_fields, nf, field_dtype, &add_h, timestep, sizes)) return 1;
  return merge_h_enqueue(c, who, d_fields, -1, timestep, add_h, compat, blur, stream ? (hipStream_t)stream : c->stream);
}
