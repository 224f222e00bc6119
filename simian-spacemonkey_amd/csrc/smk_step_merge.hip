// smk_step_merge.hip -- the multi-field step (fields + G, normals of the summed gradient) made INSIDE the time-step ring
// (smk.h: smk_merge_timestep, smk_upload_timestep_fields_device; DESIGN.md 3b "Merged fields of a step").
//
// MetaVolume::mergeMV with addG (MetaVolume.cpp:1109-1268) is a host program that runs before the renderer starts.  A step
// whose fields are new on the device -- the first nelts - 1 channels of a blend of two resident steps, or what a simulation
// left in device memory, one array per field -- gets here what smk_merge_fields_device / smk_merge_fields_f32_device (and, in
// a u16 ring, smk_quantize_u16_device) and smk_upload_timestep_device would make of them, bit for bit, as two kernels on the
// caller's stream that write the packed voxels of a ring slot: no scratch arrays, no host wait.
//
// The stencil is the six face neighbours of every field, one difference per field and axis.  Both kernels read straight
// through the caches, no LDS tile: a lane owns one 16-byte unit of the stored box (one f32 voxel, or two 8-byte voxels) and
// marches through the slices of its tile, a workgroup MG_UX units of MG_TY rows of MG_TZ slices (mg_march).  A packed source
// is read in whole units.
//   pass 1 (smk_k_merge_max):   the magnitude of the summed gradient of every interior voxel -> its maximum (u8: of all, float
//          rings: of the finite ones), one ordered-int atomicMax per wave into the OUTPUT slot's word (TimeStep::pass1_words),
//          which a one-lane kernel seeded on the stream; a capped grid strides over the tiles;
//   pass 2 (smk_k_merge_write): the gradient again, G and the normal, and one 16-byte store of the unit (and the normal word of
//          a four-channel f32 voxel).
// The arithmetic is smk_prep.hip's, through smk_prep_device.h; the packed voxel is smk_packed.h's.
// Instances of the two kernels over parameter types of their own serve sharded contexts (MergeShardParams: a packed step of
// the ring) and a decomposed simulation's own dense blocks of the volume (MergeBlockParams: smk_block_extremes_device,
// smk_upload_timestep_fields_block_device).
#include <limits.h>

#include <algorithm>

#include "smk_step_stencil.h"

namespace {

// where the fields come from: dense arrays of a type (SRC is their smk_dtype), or the channels of a slot's packed voxels (SRC_PK_*)

constexpr int MG_UX = 64, MG_TY = 4, MG_TZ = 4;  // a workgroup's tile: units in x (a wave per row), rows, slices
static_assert(MG_UX * MG_TY == 256, "a lane per unit of a slice of the tile");
constexpr unsigned MG_MAX_BLOCKS = 2048;  // pass 1's grid: 8 workgroups for each of 256 CUs (its atomics land on one cache line)

struct MergeParams {
  const void *src;    // the source slot's packed voxels [D2][D1][D0] ...
  const void *f[3];   // ... or the dense fields [N2][N1][N0], one array each
  void *out;          // the output slot's packed voxels
  uint32_t *nrm;      // its separate normal words (four-channel f32 with normals), else null
  int *mx;            // the output slot's word: the maximum magnitude, ordered-int
  int N[3], D[3];     // the volume; the stored box (origin 0: an unsharded context), D >= N with a pad column or row of 8-byte
                      // voxels.  The kernels rely on D[2] == N[2], on D == N for f32 voxels and on an even D[0] otherwise
  int normals;
  int ux, uy, ntiles;  // tiles per row of tiles, per slice of tiles, in all
};

// The SHARD instances (smk.h: smk_step_extremes_device, smk_merge_timestep_shard): the stored box lies anywhere in the volume.
// Units, tiles and every index into the slots stay LOCAL to the stored box (a unit of two 8-byte voxels starts on an even
// local x whatever the parity of O[0]); the border of the volume and its pad are decided on GLOBAL voxels O + local.  Pass 1
// takes the region's voxels alone and leaves its maximum in the caller's eight words; pass 2 reads the combined word, and
// writes zeros (normal 128) outside the valid box: a voxel on a face of the stored box that is no face of the volume has a
// neighbour this context does not hold.  A parameter TYPE of its own: the unsharded instances' code is what it was.
struct MergeShardParams : MergeParams {
  SmkShardBox B;
  int *words_out;       // pass 1: the export
  const int *words_in;  // pass 2: the combined maximum
};
// The BLOCK instances (smk.h: smk_block_extremes_device, smk_upload_timestep_fields_block_device): shard instances whose fields
// are a rank's own dense blocks of the volume, all laid out by one smk_block that lies anywhere.  Units, tiles, the region, the
// valid box and every index into the slot are the shard's; only the SOURCE differs: a voxel is read when it lies inside
// C = block ∩ stored box ∩ volume, at (local - bo) through the block's pitches (StencilBlockSrc: bo, c0, c1, py, pz).  Again a
// parameter type of its own
struct MergeBlockParams : MergeShardParams, StencilBlockSrc {};

constexpr int mg_vpu(int SRC) { return stencil_ring(SRC) == SMK_F32 ? 1 : 2;  }  // voxels per 16-byte unit

// The fields of the voxels of unit U of row Y of slice Z as they are stored -- a byte, a 16-bit value or a float's word each --:
// r[c][e], voxel c of the unit, field e.  A unit outside the stored box (and a dense voxel outside the volume) is zeros and is
// never read: no interior voxel has such a neighbour
template <int SRC, int NF, class PT>
__device__ __forceinline__ void mg_cell(const PT &P, int U, int Y, int Z, uint32_t r[][NF]) {
  constexpr int VPU = mg_vpu(SRC);
#pragma unroll
  for (int c = 0; c < VPU; ++c)
#pragma unroll
    for (int e = 0; e < NF; ++e) r[c][e] = 0u;
  if (U < 0 || U * VPU >= P.D[0] || Y < 0 || Y >= P.D[1] || Z < 0 || Z >= P.D[2]) return;
  if (SRC == SRC_PK_F32) {
    const uint4 v = ((const uint4 *)P.src)[((size_t)Z * P.D[1] + Y) * P.D[0] + U];
#pragma unroll
    for (int e = 0; e < NF; ++e) r[0][e] = e == 0 ? v.x : e == 1 ? v.y : v.z;
  } else if (SRC == SRC_PK_U8 || SRC == SRC_PK_U16) {  // two voxels (D[0] is even): their first words are .x and .z
    const uint4 v = ((const uint4 *)P.src)[((size_t)Z * P.D[1] + Y) * (size_t)(P.D[0] >> 1) + U];
#pragma unroll
    for (int c = 0; c < VPU; ++c) {
      const uint32_t w0 = c ? v.z : v.x;
#pragma unroll
      for (int e = 0; e < NF; ++e)
        r[c][e] = SRC == SRC_PK_U8 ? smk_u8_ch(w0, e) : e == 0 ? smk_vox8_c0<SMK_U16>(w0) : smk_vox8_c1<SMK_U16>(w0);
    }
  } else if constexpr (stencil_block<PT>) {  // dense fields of a block: the voxels inside C, through the pitches
    if (Y < P.c0[1] || Y >= P.c1[1] || Z < P.c0[2] || Z >= P.c1[2]) return;
    const size_t row = (size_t)(Z - P.bo[2]) * (size_t)P.pz + (size_t)(Y - P.bo[1]) * (size_t)P.py;
#pragma unroll
    for (int c = 0; c < VPU; ++c) {
      const int X = U * VPU + c;
      if (X < P.c0[0] || X >= P.c1[0]) continue;
      const size_t o = row + (size_t)(X - P.bo[0]);
#pragma unroll
      for (int e = 0; e < NF; ++e)
        r[c][e] = SRC == SMK_U8 ? (uint32_t)((const unsigned char *)P.f[e])[o]
                : SRC == SMK_U16 ? (uint32_t)((const unsigned short *)P.f[e])[o] : ((const uint32_t *)P.f[e])[o];
    }
  } else {  // dense fields, read at their element size
    if (Y >= P.N[1]) return;
#pragma unroll
    for (int c = 0; c < VPU; ++c) {
      const int X = U * VPU + c;
      if (X >= P.N[0]) continue;
      const size_t o = ((size_t)Z * P.N[1] + Y) * P.N[0] + X;
#pragma unroll
      for (int e = 0; e < NF; ++e)
        r[c][e] = SRC == SMK_U8 ? (uint32_t)((const unsigned char *)P.f[e])[o]
                : SRC == SMK_U16 ? (uint32_t)((const unsigned short *)P.f[e])[o] : ((const uint32_t *)P.f[e])[o];
    }
  }
}

// ... as the float the gradient is taken of: (float)v of an integer, unscaled (differences and their sums are exact)
template <int SRC>
__device__ __forceinline__ float mg_val(uint32_t r) {
  return stencil_ring(SRC) == SMK_F32 ? __uint_as_float(r) : (float)r;
}

// A lane's march through the MG_TZ slices of its tile at unit U of row Y: per slice visit(Z, g, r) with the summed gradients
// g[c] of the unit's voxels (0 on the volume's 1-voxel border and outside the volume) and their fields r[c].  The units before
// and behind come along in registers from slice to slice; the neighbours in the row are the neighbouring lanes' units (a wave
// is a row of the tile: every lane of it must be here), which only the wave's first and last lane have to load; the units
// above and below are loaded.  That makes three loads of a unit per unit where a plain stencil makes seven
template <int SRC, int NF, class PT, class Visit>
__device__ __forceinline__ void mg_march(const PT &P, int U, int Y, int z0, Visit visit) {
  constexpr int VPU = mg_vpu(SRC);
  const int lane = threadIdx.x & 63;
  uint32_t zm[VPU][NF], c0[VPU][NF], zp[VPU][NF];
  mg_cell<SRC, NF>(P, U, Y, z0 - 1, zm);
  mg_cell<SRC, NF>(P, U, Y, z0, c0);
  for (int tz = 0; tz < MG_TZ; ++tz) {
    const int Z = z0 + tz;
    if (Z >= P.D[2]) break;  // (the whole workgroup)
    uint32_t ym[VPU][NF], yp[VPU][NF], xl[NF], xr[NF];
    mg_cell<SRC, NF>(P, U, Y, Z + 1, zp);
    mg_cell<SRC, NF>(P, U, Y - 1, Z, ym);
    mg_cell<SRC, NF>(P, U, Y + 1, Z, yp);
#pragma unroll
    for (int e = 0; e < NF; ++e) {
      xl[e] = (uint32_t)__shfl_up((int)c0[VPU - 1][e], 1);
      xr[e] = (uint32_t)__shfl_down((int)c0[0][e], 1);
    }
    if (lane == 0 || lane == 63) {
      uint32_t t[VPU][NF];
      mg_cell<SRC, NF>(P, lane ? U + 1 : U - 1, Y, Z, t);
#pragma unroll
      for (int e = 0; e < NF; ++e) {
        if (lane) xr[e] = t[0][e];
        else xl[e] = t[VPU - 1][e];
      }
    }
    float g[VPU][3];
#pragma unroll
    for (int c = 0; c < VPU; ++c) {
      merge_grad_zero(g[c]);
      if (is_border(P.N[0], P.N[1], P.N[2], stencil_glob(P, 2, Z), stencil_glob(P, 1, Y), stencil_glob(P, 0, U * VPU + c))) continue;
#pragma unroll
      for (int e = 0; e < NF; ++e)
        merge_grad_add(g[c], mg_val<SRC>(c == VPU - 1 ? xr[e] : c0[(c + 1) % VPU][e]), mg_val<SRC>(c == 0 ? xl[e] : c0[(c + VPU - 1) % VPU][e]),
                       mg_val<SRC>(yp[c][e]), mg_val<SRC>(ym[c][e]), mg_val<SRC>(zp[c][e]), mg_val<SRC>(zm[c][e]));
    }
    visit(Z, g, c0);
#pragma unroll
    for (int c = 0; c < VPU; ++c)
#pragma unroll
      for (int e = 0; e < NF; ++e) {
        zm[c][e] = c0[c][e];
        c0[c][e] = zp[c][e];
      }
  }
}

// tile -> its first unit, row and slice
__device__ __forceinline__ void mg_tile(const MergeParams &P, int tile, int &u0, int &y0, int &z0) {
  const int bz = tile / P.uy, r = tile - bz * P.uy, by = r / P.ux;
  u0 = (r - by * P.ux) * MG_UX;
  y0 = by * MG_TY;
  z0 = bz * MG_TZ;
}

__global__ __launch_bounds__(64) void smk_k_merge_seed(int *mx) {
  if (threadIdx.x == 0) *mx = MERGE_MAX_SEED;
}

// the eight words of an export (smk.h, smk_step_extremes_device): the maximum, then seven unused words
__global__ __launch_bounds__(64) void smk_k_merge_seed_words(int *w) {
  if (threadIdx.x < 8) w[threadIdx.x] = threadIdx.x ? INT_MIN : MERGE_MAX_SEED;
}

template <int SRC, int NF, class PT = MergeParams>
__global__ __launch_bounds__(256) void smk_k_merge_max(const PT P) {
  constexpr int VPU = mg_vpu(SRC);
  const int tu = threadIdx.x % MG_UX, ty = threadIdx.x / MG_UX;
  int m = MERGE_MAX_SEED;
  for (int tile = blockIdx.x; tile < P.ntiles; tile += gridDim.x) {
    int u0, y0, z0;
    mg_tile(P, tile, u0, y0, z0);
    if constexpr (stencil_shard<PT>) {  // a tile of halo voxels alone has nothing to add (the whole workgroup skips it)
      if (u0 * VPU >= P.B.r1[0] || (u0 + MG_UX) * VPU <= P.B.r0[0] || y0 >= P.B.r1[1] || y0 + MG_TY <= P.B.r0[1] || z0 >= P.B.r1[2] ||
          z0 + MG_TZ <= P.B.r0[2])
        continue;
    }
    const int U = u0 + tu, Y = y0 + ty;
    mg_march<SRC, NF>(P, U, Y, z0, [&](int Z, const float g[][3], const uint32_t r[][NF]) {
#pragma unroll
      for (int c = 0; c < VPU; ++c) {
        const int X = U * VPU + c;
        if constexpr (stencil_shard<PT>) {  // the region's voxels alone
          if (X < P.B.r0[0] || X >= P.B.r1[0] || Y < P.B.r0[1] || Y >= P.B.r1[1] || Z < P.B.r0[2] || Z >= P.B.r1[2]) continue;
        }
        if (is_border(P.N[0], P.N[1], P.N[2], stencil_glob(P, 2, Z), stencil_glob(P, 1, Y), stencil_glob(P, 0, X))) continue;  // (and everything outside the volume)
        const float mag = merge_mag(g[c]);
        m = stencil_ring(SRC) == SMK_U8 ? merge_max_take(m, mag) : merge_max_take_f32(m, mag);
      }
    });
  }
  m = wave_max(m);
  if constexpr (stencil_shard<PT>) {
    if ((threadIdx.x & 63) == 0) atomicMax(P.words_out, m);
  } else {
    if ((threadIdx.x & 63) == 0) atomicMax(P.mx, m);
  }
}

// the packed voxel of the output at column X of row Y from its summed gradient g and its fields r: w[0..1] of an 8-byte ring,
// w[0..3] of f32; nw: the normal word
template <int SRC, int NF, class PT>
__device__ __forceinline__ void mg_voxel(const PT &P, int X, int Y, int Z, const float gin[3], const uint32_t r[NF], float maxm, uint32_t w[4],
                                         uint32_t &nw) {
  constexpr int RING = stencil_ring(SRC);
  nw = SMK_NRM_NONE;
  if (stencil_glob(P, 0, X) >= P.N[0] || stencil_glob(P, 1, Y) >= P.N[1]) {  // the pad column or row of an 8-byte box: zeros, as after an upload
    w[0] = w[1] = w[2] = w[3] = 0u;
    return;
  }
  if constexpr (stencil_shard<PT>) {  // the rim: zeros that carry no normal (a four-channel f32 voxel's goes to the separate buffer)
    if (X < P.B.v0[0] || X >= P.B.v1[0] || Y < P.B.v0[1] || Y >= P.B.v1[1] || Z < P.B.v0[2] || Z >= P.B.v1[2]) {
      w[0] = w[1] = w[2] = w[3] = 0u;
      if (RING != SMK_F32) w[1] = SMK_NRM_NONE;
      else if (NF + 1 <= 3) w[3] = SMK_NRM_NONE;
      return;
    }
  }
  float g[3] = {gin[0], gin[1], gin[2]};
  const float mag = merge_mag(g);
  if (P.normals) {
    unsigned char n[3];
    if (RING == SMK_U8) nrm_store(g, n);
    else nrm_store_f32(g, n);  // (u16: the float entry's normals, made from the floats before any quantisation)
    nw = smk_nrm_word(n[0], n[1], n[2]);
  }
  if (RING == SMK_U8) {  // (the fields are copied, on the border too)
    unsigned char q[NF + 1];
#pragma unroll
    for (int e = 0; e < NF; ++e) q[e] = (unsigned char)r[e];
    q[NF] = merge_gmag_u8(mag, maxm);
    const uint2 v = smk_pack_u8(q, NF + 1, nw);
    w[0] = v.x, w[1] = v.y;
  } else if (RING == SMK_U16) {
    unsigned short s[NF + 1];
#pragma unroll
    for (int e = 0; e < NF; ++e) s[e] = (unsigned short)r[e];
    s[NF] = quant_u16(merge_g_f32(mag, maxm));  // smk_quantize_u16_device of the float G
    const uint2 v = smk_pack_u16(s, NF + 1, nw);
    w[0] = v.x, w[1] = v.y;
  } else {
    float f[NF + 1];
#pragma unroll
    for (int e = 0; e < NF; ++e) f[e] = __uint_as_float(r[e]);  // raw words: NaN payloads and -0 travel
    f[NF] = merge_g_f32(mag, maxm);
    const uint4 v = smk_pack_f32(f, NF + 1, nw, NF + 1 <= 3);
    w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
  }
}

template <int SRC, int NF, class PT = MergeParams>
__global__ __launch_bounds__(256) void smk_k_merge_write(const PT P) {
  constexpr int VPU = mg_vpu(SRC);
  float maxm;  // (a shard's comes combined from the caller's words)
  if constexpr (stencil_shard<PT>) maxm = o2f(P.words_in[0]);
  else maxm = o2f(*P.mx);
  int u0, y0, z0;
  mg_tile(P, blockIdx.x, u0, y0, z0);
  const int U = u0 + threadIdx.x % MG_UX, Y = y0 + threadIdx.x / MG_UX;
  const bool stored = U * VPU < P.D[0] && Y < P.D[1];  // (a lane outside the box stays for its neighbours' sake)
  mg_march<SRC, NF>(P, U, Y, z0, [&](int Z, const float g[][3], const uint32_t r[][NF]) {
    if (!stored) return;
    const size_t o = ((size_t)Z * P.D[1] + Y) * (size_t)(P.D[0] / VPU) + U;  // the unit
    uint32_t w[4], nw;
    if (VPU == 1) {
      mg_voxel<SRC, NF>(P, U, Y, Z, g[0], r[0], maxm, w, nw);
      if (NF == 3 && P.nrm) P.nrm[o] = nw;
    } else {
      uint32_t hi[4];
      mg_voxel<SRC, NF>(P, 2 * U, Y, Z, g[0], r[0], maxm, w, nw);
      mg_voxel<SRC, NF>(P, 2 * U + 1, Y, Z, g[VPU - 1], r[VPU - 1], maxm, hi, nw);
      w[2] = hi[0], w[3] = hi[1];
    }
    ((uint4 *)P.out)[o] = make_uint4(w[0], w[1], w[2], w[3]);
  });
}

// The seed and pass 1 (PASS_1: into the slot's word, a shard's and a block's into the caller's words), pass 2, or both, of the
// instance that reads the ring's type -- a packed step of the ring (PACKED) or dense fields -- with the series' fields
template <bool PACKED, class PT>
hipError_t launch_merge(const smk_ctx *c, const PT &P, int passes, hipStream_t s) {
  return stencil_dispatch<PACKED>(c->dtype, c->nelts - 1, [&](auto src, auto nf) {
    constexpr int SRC = decltype(src)::value, NF = decltype(nf)::value;
    if (passes & PASS_1) {
      if constexpr (stencil_shard<PT>) hipLaunchKernelGGL(smk_k_merge_seed_words, dim3(1), dim3(64), 0, s, P.words_out);
      else hipLaunchKernelGGL(smk_k_merge_seed, dim3(1), dim3(64), 0, s, P.mx);
      hipLaunchKernelGGL((smk_k_merge_max<SRC, NF, PT>), dim3(std::min<unsigned>((unsigned)P.ntiles, MG_MAX_BLOCKS)), dim3(256), 0, s, P);
    }
    if (passes & PASS_2) hipLaunchKernelGGL((smk_k_merge_write<SRC, NF, PT>), dim3((unsigned)P.ntiles), dim3(256), 0, s, P);
    return hipGetLastError();
  });
}

// what both entries refuse before they look at their data (smk_step_stencil_refusals)
StencilEntry merge_entry(const smk_ctx *c, const char *who) {
  char nelts_why[112] = "";
  const int top = c->dtype == SMK_U16 ? 3 : 4;
  if (c->nelts < 2) snprintf(nelts_why, sizeof nelts_why, "the series has nelts %d: a multi-field step is at least one field and G (nelts >= 2)", c->nelts);
  else if (c->nelts > top) snprintf(nelts_why, sizeof nelts_why, "internal: nelts %d of a voxel type that holds %d channels", c->nelts, top);
  return {who, "the stencil reaches 1 voxel beyond region + halo, and G is scaled by the whole volume's maximum", nelts_why,
          "smk_merge_fields_device"};
}

// What every instance takes of the context: the volume, the stored box and its tiles, and with `fields` the series' dense
// fields; no packed source and no output yet.  More than 2^31 tiles (2^42 voxels: no ring holds such a step, so the place of
// this refusal before the frame's is moot) are refused in the words of the entries of the whole volume (`whole`), or of the
// shard and block entries
int merge_common(smk_ctx *c, const char *who, bool whole, const void *const *fields, MergeParams &P) {
  const int VPU = c->dtype == SMK_F32 ? 1 : 2, nf = c->nelts - 1;
  const long long ux = (c->D[0] / VPU + MG_UX - 1) / MG_UX, uy = (c->D[1] + MG_TY - 1) / MG_TY, uz = (c->D[2] + MG_TZ - 1) / MG_TZ;
  if (ux * uy * uz > 0x7fffffffLL) {
    if (whole) FAIL(c, "%s: a %dx%dx%d volume has more than 2^31 tiles", who, c->N[0], c->N[1], c->N[2]);
    FAIL(c, "%s: a %dx%dx%d stored box has more than 2^31 tiles", who, c->D[0], c->D[1], c->D[2]);
  }
  P.src = nullptr;
  for (int e = 0; e < 3; ++e) P.f[e] = fields && e < nf ? fields[e] : nullptr;
  P.out = nullptr;
  P.nrm = nullptr;
  P.mx = nullptr;
  for (int a = 0; a < 3; ++a) {
    P.N[a] = c->N[a];
    P.D[a] = c->D[a];
  }
  P.normals = c->have_normals ? 1 : 0;
  P.ux = (int)ux;
  P.uy = (int)(ux * uy);
  P.ntiles = (int)(ux * uy * uz);
  return 0;
}

// the two passes inside the producer frame; ksrc: the source slot, or -1 (dense fields)
int merge_enqueue(smk_ctx *c, const char *who, const void *const *fields, int ksrc, int step_out, hipStream_t s) {
  MergeParams P;
  if (merge_common(c, who, true, fields, P)) return 1;
  return smk_step_produce(c, who, step_out, ksrc, -1, s, [&](TimeStep &T, const TimeStep *S, const TimeStep *) -> int {
    P.src = S ? S->vox : nullptr;
    P.out = T.vox;
    P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
    P.mx = T.pass1_words;
    HIPCHK(c, S ? launch_merge<true>(c, P, PASS_1 | PASS_2, s) : launch_merge<false>(c, P, PASS_1 | PASS_2, s));
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------- the shard entries

constexpr int MG_REACH = 1;  // the six face neighbours

StencilEntry merge_shard_entry(const smk_ctx *c, const char *who) {
  StencilEntry E = merge_entry(c, who);
  E.sharded_why = "";
  return E;
}

// the shard's parameters with the packed step S as the source (B: the region, and the result's valid box)
int merge_shard_params(smk_ctx *c, const char *who, const TimeStep &S, MergeShardParams &P) {
  if (merge_common(c, who, false, nullptr, P)) return 1;
  P.src = S.vox;
  smk_step_shard_box(c, S, MG_REACH, P.B);
  P.words_out = nullptr;
  P.words_in = nullptr;
  return 0;
}

// ---------------------------------------------------------------------------------------------- the block entries

// What both block entries refuse, and the shard's parameters with the block's fields as the source (B: the region, and C shrunk
// by the reach as the result's valid box).  step_out: null for the export
int merge_block_params(smk_ctx *c, const char *who, const int *step_out, const void *const *d_fields, int nf, smk_dtype dt, const smk_block *b,
                       SmkBlockView &V, MergeBlockParams &P) {
  if (smk_step_block_refusals(c, merge_shard_entry(c, who), MG_REACH, step_out, b, V)) return 1;
  if (stencil_fields_refusals(c, who, d_fields, nf, dt, nullptr, -1, nullptr)) return 1;
  if (merge_common(c, who, false, d_fields, P)) return 1;
  stencil_block_src(c, b, V, P);
  smk_step_block_box(c, V, MG_REACH, P.B);
  P.words_out = nullptr;
  P.words_in = nullptr;
  return 0;
}

}  // namespace

int smk_merge_block_extremes_enqueue(smk_ctx *c, const char *who, const void *const *d_fields, int nf, smk_dtype dtype, const smk_block *b,
                                     void *d_words, hipStream_t s) {
  SmkBlockView V;
  MergeBlockParams P;
  if (merge_block_params(c, who, nullptr, d_fields, nf, dtype, b, V, P)) return 1;
  P.words_out = (int *)d_words;
  HIPCHK(c, launch_merge<false>(c, P, PASS_1, s));
  return 0;
}

extern "C" int smk_upload_timestep_fields_block_device(smk_ctx *c, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                                       const smk_block *b, const void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_fields_block_device";
  HIPCHK(c, hipSetDevice(c->device));
  SmkBlockView V;
  MergeBlockParams P;
  if (merge_block_params(c, who, &timestep, d_fields, nf, field_dtype, b, V, P) || stencil_words_refusals(c, who, d_words)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, timestep, -1, -1, s, [&](TimeStep &T, const TimeStep *, const TimeStep *) -> int {
    P.out = T.vox;
    P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
    P.words_in = (const int *)d_words;
    HIPCHK(c, launch_merge<false>(c, P, PASS_2, s));
    smk_step_block_done(c, V, MG_REACH, P.B, T);
    return 0;
  });
}

int smk_merge_extremes_enqueue(smk_ctx *c, const char *who, int step_src, void *d_words, hipStream_t s) {
  int ksrc = -1;
  if (smk_step_shard_refusals(c, merge_shard_entry(c, who), MG_REACH, step_src, nullptr, &ksrc)) return 1;
  MergeShardParams P;
  if (merge_shard_params(c, who, c->ts[(size_t)ksrc], P)) return 1;
  P.words_out = (int *)d_words;
  return smk_step_read(c, ksrc, -1, s, [&]() -> int {
    HIPCHK(c, launch_merge<true>(c, P, PASS_1, s));
    return 0;
  });
}

extern "C" int smk_merge_timestep_shard(smk_ctx *c, int step_src, int step_out, const void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_merge_timestep_shard";
  HIPCHK(c, hipSetDevice(c->device));
  int ksrc = -1;
  if (smk_step_shard_refusals(c, merge_shard_entry(c, who), MG_REACH, step_src, &step_out, &ksrc)) return 1;
  MergeShardParams P;
  if (stencil_words_refusals(c, who, d_words) || merge_shard_params(c, who, c->ts[(size_t)ksrc], P)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, step_out, ksrc, -1, s, [&](TimeStep &T, const TimeStep *S, const TimeStep *) -> int {
    P.out = T.vox;
    P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
    P.words_in = (const int *)d_words;
    HIPCHK(c, launch_merge<true>(c, P, PASS_2, s));
    smk_step_shard_done(c, *S, MG_REACH, P.B, T);
    return 0;
  });
}

extern "C" int smk_merge_timestep(smk_ctx *c, int step_src, int step_out, void *stream) {
  if (!c) return 1;
  const char *who = "smk_merge_timestep";
  HIPCHK(c, hipSetDevice(c->device));
  int ksrc = -1;
  if (smk_step_stencil_refusals(c, merge_entry(c, who), step_out, &step_src, &ksrc)) return 1;
  return merge_enqueue(c, who, nullptr, ksrc, step_out, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_upload_timestep_fields_device(smk_ctx *c, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                                 int sx, int sy, int sz, void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_fields_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (smk_step_stencil_refusals(c, merge_entry(c, who), timestep, nullptr, nullptr)) return 1;
  const int sizes[3] = {sx, sy, sz};
  if (stencil_fields_refusals(c, who, d_fields, nf, field_dtype, nullptr, timestep, sizes)) return 1;
  return merge_enqueue(c, who, d_fields, -1, timestep, stream ? (hipStream_t)stream : c->stream);
}
