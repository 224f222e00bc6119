// smk_step_derive.hip -- V, G, H and normals of a scalar made INSIDE the time-step ring (smk.h: smk_derive_timestep,
// smk_upload_timestep_scalar_device; DESIGN.md 3b "Derivatives of a step").
//
// genVGH's makeVGH (genVGH/main.cpp:56-182) and MetaVolume::normalsVGH (MetaVolume.cpp:1274-1324) are host programs that run
// before the renderer starts.  A step whose scalar is new on the device -- channel 0 of a blend of two resident steps, or what
// a simulation left in device memory -- gets here what smk_make_vgh_device, smk_quantize_u16_device, smk_normals_*_device and
// smk_upload_timestep_device would make of it, bit for bit, as two kernels on the caller's stream that write the packed
// voxels of a ring slot: no scratch arrays, no host wait.
//
// Both kernels work on tiles of DV_TX x DV_TY x DV_TZ voxels of the stored box from an LDS copy of the scalar AS FLOATS with
// a 2-voxel apron on every side: H reads the gradients of the six neighbours, each a central difference (2 voxels), and a
// blurred normal reads the differences of the OUTPUT V channel at the 27 neighbours (2 voxels again).
//   pass 1 (smk_k_derive_stats): gm, hs and the scalar of every interior voxel -> the six extremes, ordered-int atomics into
//          the OUTPUT slot's words (TimeStep::pass1_words), which a one-thread kernel seeded on the stream;
//   pass 2 (smk_k_derive_write): the reference's +-1e8 seeds applied to those words, the scaled V of every tile voxel (0 on the
//          volume's border and outside it) into a second LDS tile, then per voxel gm and hs again, the scaling, the normal
//          from the V tile, and one 8- or 16-byte store of the packed voxel.
// The arithmetic is smk_prep.hip's, through smk_prep_device.h; the packed voxel is smk_packed.h's.
// Instances of the two kernels over parameter types of their own serve sharded contexts (DeriveShardParams: a packed step of
// the ring) and a decomposed simulation's own dense block of the volume (DeriveBlockParams: smk_block_extremes_device,
// smk_upload_timestep_scalar_block_device).
#include <limits.h>

#include <algorithm>

#include "smk_step_stencil.h"

namespace {

// where the scalar comes from: a dense array of a type (SRC is its smk_dtype), or channel 0 of a slot's packed voxels (SRC_PK_*)

constexpr int DV_TX = 32, DV_TY = 8, DV_TZ = 8, DV_AP = 2;
constexpr int DV_LX = DV_TX + 2 * DV_AP, DV_LY = DV_TY + 2 * DV_AP, DV_LZ = DV_TZ + 2 * DV_AP;
constexpr int DV_LN = DV_LX * DV_LY * DV_LZ;  // 5184 floats
constexpr int DV_SY = DV_LX, DV_SZ = DV_LX * DV_LY;
static_assert(DV_TX * DV_TY == 256 && DV_TX % 2 == 0 && DV_AP % 2 == 0, "a thread per (x, y) of the tile; tile rows start on even x");

struct DeriveParams {
  const void *src;  // the dense scalar [N2][N1][N0], or the source slot's packed voxels [D2][D1][D0]
  void *out;        // the output slot's packed voxels
  VghStats *st;     // the output slot's extremes
  int N[3], D[3];   // the volume; the stored box (origin 0: an unsharded context), D >= N with a pad column or row of 8-byte voxels.
                    // The kernels rely on D[2] == N[2], on D == N for f32 voxels and on an even D[0] otherwise: smk_step_stencil_refusals checks
  int compat, blur, normals;
};

// The SHARD instances (smk.h: smk_step_extremes_device, smk_derive_timestep_shard): the stored box lies anywhere in the volume.
// Tiles and every index into S, V and the slots stay LOCAL to the stored box, so a 16-byte unit of two 8-byte voxels starts
// on an even local x whatever the parity of O[0]; the border of the volume, its interior and its pad are decided on GLOBAL
// voxels O + local.  Pass 1 takes the region's voxels alone and leaves its extremes in the caller's eight words, every
// minimum complemented; pass 2 reads the combined words, and writes zeros (normal 128) outside the valid box: what lies
// within `reach` of a face of the stored box that is no face of the volume was made from voxels this context does not hold.
// A parameter TYPE of its own: the unsharded instances' code is what it was.
struct DeriveShardParams : DeriveParams {
  SmkShardBox B;
  int *words_out;       // pass 1: the export
  const int *words_in;  // pass 2: the combined extremes
};
// The BLOCK instances (smk.h: smk_block_extremes_device, smk_upload_timestep_scalar_block_device): shard instances whose scalar
// is a rank's own dense block of the volume, lying anywhere.  Tiles, the region, the valid box and every index into S, V and the
// slot are the shard's; only the SOURCE differs: a voxel is held when it lies inside C = block ∩ stored box ∩ volume, and it is
// read at (local - bo) through the block's pitches (StencilBlockSrc: bo, c0, c1, py, pz).  Again a parameter type of its own
struct DeriveBlockParams : DeriveShardParams, StencilBlockSrc {};

// the tile of the scalar around (x0, y0, z0), apron included; what lies outside the volume is not data: 0, and never used
template <int SRC, class PT>
__device__ __forceinline__ void dv_load_tile(const PT &P, int x0, int y0, int z0, float *S) {
  if (SRC == SRC_PK_U8 || SRC == SRC_PK_U16) {  // two 8-byte voxels per 16-byte unit (x0 - DV_AP is even, and so is D[0])
    constexpr int UPR = DV_LX / 2;
    for (int u = threadIdx.x; u < UPR * DV_LY * DV_LZ; u += 256) {
      const int cu = u % UPR, row = u / UPR, ly = row % DV_LY, lz = row / DV_LY;
      const int X = x0 - DV_AP + 2 * cu, Y = y0 - DV_AP + ly, Z = z0 - DV_AP + lz;
      float a = 0.f, b = 0.f;
      if (stencil_held(P, X, Y, Z)) {
        const uint4 v = ((const uint4 *)P.src)[(((size_t)Z * P.D[1] + Y) * P.D[0] + X) >> 1];
        constexpr int DT = SRC == SRC_PK_U8 ? SMK_U8 : SMK_U16;
        a = (float)smk_vox8_c0<DT>(v.x);
        if (stencil_glob(P, 0, X) + 1 < P.N[0]) b = (float)smk_vox8_c0<DT>(v.z);
      }
      S[row * DV_LX + 2 * cu] = a;
      S[row * DV_LX + 2 * cu + 1] = b;
    }
  } else {
    for (int t = threadIdx.x; t < DV_LN; t += 256) {
      const int lx = t % DV_LX, row = t / DV_LX, ly = row % DV_LY, lz = row / DV_LY;
      const int X = x0 - DV_AP + lx, Y = y0 - DV_AP + ly, Z = z0 - DV_AP + lz;
      float a = 0.f;
      if (stencil_held(P, X, Y, Z)) {
        if (SRC == SRC_PK_F32) {
          a = __uint_as_float(((const uint4 *)P.src)[((size_t)Z * P.D[1] + Y) * P.D[0] + X].x);
        } else {
          size_t o;
          if constexpr (stencil_block<PT>) o = (size_t)(Z - P.bo[2]) * (size_t)P.pz + (size_t)(Y - P.bo[1]) * (size_t)P.py + (size_t)(X - P.bo[0]);
          else o = ((size_t)Z * P.N[1] + Y) * P.N[0] + X;
          a = SRC == SMK_U8 ? (float)((const unsigned char *)P.src)[o] : SRC == SMK_U16 ? (float)((const unsigned short *)P.src)[o] : ((const float *)P.src)[o];
        }
      }
      S[t] = a;
    }
  }
}

// un-normalised central differences at tile index l (genVGH/main.cpp:86-88): x, then y, then z
__device__ __forceinline__ void dv_grad(const float *S, int l, float g[3]) {
  g[0] = S[l + 1] - S[l - 1];
  g[1] = S[l + DV_SY] - S[l - DV_SY];
  g[2] = S[l + DV_SZ] - S[l - DV_SZ];
}

// ... of a neighbour, the voxel (Z, Y, X) of the VOLUME: zero on the volume's 1-voxel border (:79-84)
template <class PT>
__device__ __forceinline__ void dv_grad_nb(const PT &P, const float *S, int l, int Z, int Y, int X, float g[3]) {
  if (is_border(P.N[0], P.N[1], P.N[2], Z, Y, X)) g[0] = g[1] = g[2] = 0.f;
  else dv_grad(S, l, g);
}

// gm and hs of the INTERIOR voxel (Z, Y, X) of the volume at tile index l
template <class PT>
__device__ __forceinline__ void dv_gh(const PT &P, const float *S, int l, int Z, int Y, int X, float &gm, float &hs) {
  float g[3], xp[3], xm[3], yp[3], ym[3], zp[3], zm[3];
  dv_grad(S, l, g);
  dv_grad_nb(P, S, l + 1, Z, Y, X + 1, xp);
  dv_grad_nb(P, S, l - 1, Z, Y, X - 1, xm);
  dv_grad_nb(P, S, l + DV_SY, Z, Y + 1, X, yp);
  dv_grad_nb(P, S, l - DV_SY, Z, Y - 1, X, ym);
  dv_grad_nb(P, S, l + DV_SZ, Z + 1, Y, X, zp);
  dv_grad_nb(P, S, l - DV_SZ, Z - 1, Y, X, zm);
  gh_from_grads(g, xp, xm, yp, ym, zp, zm, P.compat, gm, hs);
}

__global__ __launch_bounds__(64) void smk_k_derive_seed(VghStats *st) {
  if (threadIdx.x == 0) {
    VghStats init = {ORD_POS_INF, ORD_NEG_INF, ORD_POS_INF, ORD_NEG_INF, ORD_POS_INF, ORD_NEG_INF};
    *st = init;
  }
}

// A capped grid strides over the tiles, so that the extremes reach the device words as a few ten thousand atomics whatever
// the volume's size (they all land on one cache line)
constexpr unsigned DV_STATS_BLOCKS = 2048;  // 8 workgroups for each of 256 CUs

// the eight words of an export (smk.h, smk_step_extremes_device): every minimum complemented, so that all combine by maximum
__global__ __launch_bounds__(64) void smk_k_derive_seed_words(int *w) {
  if (threadIdx.x < 8) w[threadIdx.x] = threadIdx.x >= 6 ? INT_MIN : (threadIdx.x & 1) ? ORD_NEG_INF : ~ORD_POS_INF;
}

// ... a wave's running extremes into them (every lane of the wave calls this)
__device__ __forceinline__ void dv_publish_words(VghRunning &run, int *w) {
  const int dmin = wave_min(run.dmin), dmax = wave_max(run.dmax), gmin = wave_min(run.gmin), gmax = wave_max(run.gmax), hmin = wave_min(run.hmin),
            hmax = wave_max(run.hmax);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&w[0], ~dmin);
    atomicMax(&w[1], dmax);
    atomicMax(&w[2], ~gmin);
    atomicMax(&w[3], gmax);
    atomicMax(&w[4], ~hmin);
    atomicMax(&w[5], hmax);
  }
}

template <int SRC, class PT = DeriveParams>
__global__ __launch_bounds__(256) void smk_k_derive_stats(const PT P, int gx, int gy, int ntiles) {
  __shared__ float S[DV_LN];
  const int tx = threadIdx.x % DV_TX, ty = threadIdx.x / DV_TX;
  VghRunning run;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int bx = tile % gx, by = (tile / gx) % gy, bz = tile / (gx * gy);
    const int x0 = bx * DV_TX, y0 = by * DV_TY, z0 = bz * DV_TZ;
    if constexpr (stencil_shard<PT>) {  // a tile of halo voxels alone has nothing to add (the whole workgroup skips it)
      if (x0 >= P.B.r1[0] || x0 + DV_TX <= P.B.r0[0] || y0 >= P.B.r1[1] || y0 + DV_TY <= P.B.r0[1] || z0 >= P.B.r1[2] || z0 + DV_TZ <= P.B.r0[2])
        continue;
    }
    dv_load_tile<SRC>(P, x0, y0, z0, S);
    __syncthreads();
    const int X = x0 + tx, Y = y0 + ty, GX = stencil_glob(P, 0, X), GY = stencil_glob(P, 1, Y);
    bool mine = true;
    if constexpr (stencil_shard<PT>) mine = X >= P.B.r0[0] && X < P.B.r1[0] && Y >= P.B.r0[1] && Y < P.B.r1[1];  // the region's voxels alone
    for (int tz = 0; tz < DV_TZ; ++tz) {
      const int Z = z0 + tz, GZ = stencil_glob(P, 2, Z);
      if constexpr (stencil_shard<PT>) {
        if (!mine || Z < P.B.r0[2] || Z >= P.B.r1[2]) continue;
      }
      if (is_border(P.N[0], P.N[1], P.N[2], GZ, GY, GX)) continue;  // (and everything outside the volume)
      const int l = (tz + DV_AP) * DV_SZ + (ty + DV_AP) * DV_SY + tx + DV_AP;
      float gm, hs;
      dv_gh(P, S, l, GZ, GY, GX, gm, hs);
      run.take(S[l], gm, hs);
    }
    __syncthreads();  // (the next tile overwrites S)
  }
  if constexpr (stencil_shard<PT>) dv_publish_words(run, P.words_out);
  else run.publish(P.st);
}

// std::min / std::max of <algorithm> as smk_make_vgh_device applies them to the extremes and the reference's seeds
__device__ __forceinline__ float dv_std_min(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float dv_std_max(float a, float b) { return (a < b) ? b : a; }

// OUT: the ring's dtype (smk_dtype)
template <int SRC, int OUT, class PT = DeriveParams>
__global__ __launch_bounds__(256) void smk_k_derive_write(const PT P) {
  __shared__ float S[DV_LN], V[DV_LN];
  const int x0 = blockIdx.x * DV_TX, y0 = blockIdx.y * DV_TY, z0 = blockIdx.z * DV_TZ;
  dv_load_tile<SRC>(P, x0, y0, z0, S);
  VghStats st;  // (a shard's come combined from the caller's words, the minima complemented)
  if constexpr (stencil_shard<PT>) st = {~P.words_in[0], P.words_in[1], ~P.words_in[2], P.words_in[3], ~P.words_in[4], P.words_in[5]};
  else st = *P.st;
  // the reference seeds its running min/max with +-1e8 (genVGH/main.cpp:69-72, 104-105)
  const float dmin = dv_std_min(o2f(st.dmin), 100000000.f), dmax = dv_std_max(o2f(st.dmax), -100000000.f);
  const float gmin = dv_std_min(o2f(st.gmin), 100000000.f), gmax = dv_std_max(o2f(st.gmax), -100000000.f);
  const float hmin = dv_std_min(o2f(st.hmin), 100000000.f), hmax = dv_std_max(o2f(st.hmax), -100000000.f);
  __syncthreads();
  // the OUTPUT's V channel as the normals' source: the byte (u8) or the float before any quantisation; 0 on the border
  for (int t = threadIdx.x; t < DV_LN; t += 256) {
    const int lx = t % DV_LX, row = t / DV_LX, ly = row % DV_LY, lz = row / DV_LY;
    const int X = x0 - DV_AP + lx, Y = y0 - DV_AP + ly, Z = z0 - DV_AP + lz;
    float v = 0.f;
    // (plain normals read V one voxel around the tile's own voxels, blurred ones two: the outer ring is not read then)
    const bool read = P.blur || (lx >= 1 && lx < DV_LX - 1 && ly >= 1 && ly < DV_LY - 1 && lz >= 1 && lz < DV_LZ - 1);
    if (read && !is_border(P.N[0], P.N[1], P.N[2], stencil_glob(P, 2, Z), stencil_glob(P, 1, Y), stencil_glob(P, 0, X))) {
      const double vq = affine_d(dmin, S[t], dmax, 0, 255);  // (vgh_scale's V)
      v = OUT == SMK_U8 ? (float)uc_cast(vq) : (float)(vq / 255.0);
    }
    V[t] = v;
  }
  __syncthreads();
  const int tx = threadIdx.x % DV_TX, ty = threadIdx.x / DV_TX, X = x0 + tx, Y = y0 + ty;
  if (X >= P.D[0] || Y >= P.D[1]) return;
  const int GX = stencil_glob(P, 0, X), GY = stencil_glob(P, 1, Y);
  for (int tz = 0; tz < DV_TZ; ++tz) {
    const int Z = z0 + tz, GZ = stencil_glob(P, 2, Z);
    if (Z >= P.D[2]) break;
    const size_t o = ((size_t)Z * P.D[1] + Y) * P.D[0] + X;
    if (GX >= P.N[0] || GY >= P.N[1]) {  // the pad column or row of an 8-byte box: zeros, as after an upload
      ((uint2 *)P.out)[o] = make_uint2(0u, 0u);
      continue;
    }
    if constexpr (stencil_shard<PT>) {  // the rim: zeros that carry no normal
      if (X < P.B.v0[0] || X >= P.B.v1[0] || Y < P.B.v0[1] || Y >= P.B.v1[1] || Z < P.B.v0[2] || Z >= P.B.v1[2]) {
        if (OUT == SMK_F32) ((uint4 *)P.out)[o] = make_uint4(0u, 0u, 0u, SMK_NRM_NONE);
        else ((uint2 *)P.out)[o] = make_uint2(0u, SMK_NRM_NONE);
        continue;
      }
    }
    const int l = (tz + DV_AP) * DV_SZ + (ty + DV_AP) * DV_SY + tx + DV_AP;
    unsigned char q[3] = {0, 0, 0};
    float f[3] = {0.f, 0.f, 0.f};
    if (!is_border(P.N[0], P.N[1], P.N[2], GZ, GY, GX)) {
      float gm, hs;
      dv_gh(P, S, l, GZ, GY, GX, gm, hs);
      vgh_scale(S[l], gm, hs, dmin, dmax, gmin, gmax, hmin, hmax, q, f);
    }
    uint32_t nb = SMK_NRM_NONE;
    if (P.normals) {
      float g[3];
      unsigned char n[3];
      // (Z, Y, X) -> tile index: l moved by the offset; the differences of bytes held as floats are exact
      nrm_gradient(P.blur, P.N[0], P.N[1], P.N[2], GZ, GY, GX, g, [&](int si, int sj, int sk, float s[3]) {
        dv_grad(V, l + (si - GZ) * DV_SZ + (sj - GY) * DV_SY + (sk - GX), s);
      });
      if (OUT == SMK_U8) nrm_store(g, n);
      else nrm_store_f32(g, n);
      nb = smk_nrm_word(n[0], n[1], n[2]);
    }
    if (OUT == SMK_U8) {
      ((uint2 *)P.out)[o] = smk_pack_u8(q, 3, nb);
    } else if (OUT == SMK_U16) {
      // smk_quantize_u16_device of the floats, then the pack's 8-bit unorm of the third channel
      const unsigned short s[3] = {quant_u16(f[0]), quant_u16(f[1]), quant_u16(f[2])};
      ((uint2 *)P.out)[o] = smk_pack_u16(s, 3, nb);
    } else {
      ((uint4 *)P.out)[o] = smk_pack_f32(f, 3, nb, 1);
    }
  }
}

// The seed and pass 1 (PASS_1: into the slot's extremes, a shard's and a block's into the caller's words), pass 2, or both
template <int SRC, int OUT, class PT>
hipError_t launch_derive(const PT &P, int passes, hipStream_t s) {
  const dim3 grid((unsigned)((P.D[0] + DV_TX - 1) / DV_TX), (unsigned)((P.D[1] + DV_TY - 1) / DV_TY), (unsigned)((P.D[2] + DV_TZ - 1) / DV_TZ));
  if (passes & PASS_1) {
    const long long ntiles = (long long)grid.x * grid.y * grid.z;
    if (ntiles > 0x7fffffffLL) return hipErrorInvalidValue;  // (2^31 tiles are 2^42 voxels)
    if constexpr (stencil_shard<PT>) hipLaunchKernelGGL(smk_k_derive_seed_words, dim3(1), dim3(64), 0, s, P.words_out);
    else hipLaunchKernelGGL(smk_k_derive_seed, dim3(1), dim3(64), 0, s, P.st);
    hipLaunchKernelGGL((smk_k_derive_stats<SRC, PT>), dim3((unsigned)std::min<long long>(ntiles, DV_STATS_BLOCKS)), dim3(256), 0, s, P, (int)grid.x,
                       (int)grid.y, (int)ntiles);
  }
  if (passes & PASS_2) hipLaunchKernelGGL((smk_k_derive_write<SRC, OUT, PT>), grid, dim3(256), 0, s, P);
  return hipGetLastError();
}

// ... of the instance that reads a source of type dt -- a packed step of the ring (PACKED) or a dense scalar -- and writes the
// ring's voxels.  A shard's source IS a step of the ring: its kernels have the instances of equal types alone
template <bool PACKED, class PT>
hipError_t launch_derive_src(const smk_ctx *c, const PT &P, int dt, int passes, hipStream_t s) {
  return stencil_dispatch_src<PACKED>(dt, [&](auto src) -> hipError_t {
    constexpr int SRC = decltype(src)::value;
    if constexpr (PACKED && stencil_shard<PT>) {
      return launch_derive<SRC, stencil_ring(SRC)>(P, passes, s);
    } else {
      return stencil_dispatch_src<false>(c->dtype, [&](auto out) { return launch_derive<SRC, decltype(out)::value>(P, passes, s); });
    }
  });
}

// what both entries refuse before they look at their data (smk_step_stencil_refusals)
StencilEntry derive_entry(const smk_ctx *c, const char *who) {
  char nelts_why[96] = "";
  if (c->nelts != 3) snprintf(nelts_why, sizeof nelts_why, "the series has nelts %d: V, G and H are three channels (nelts 3)", c->nelts);
  return {who, "the stencil reaches 2 voxels beyond a voxel and the scaling needs the whole volume's extremes; neither fits region + halo",
          nelts_why, "smk_make_vgh_device"};
}

// what every instance takes of the context: the volume, the stored box, the flags; no output yet
void derive_common(const smk_ctx *c, const void *src, int compat, int blur, DeriveParams &P) {
  P.src = src;
  P.out = nullptr;
  P.st = nullptr;
  for (int a = 0; a < 3; ++a) {
    P.N[a] = c->N[a];
    P.D[a] = c->D[a];
  }
  P.compat = compat ? 1 : 0;
  P.blur = blur ? 1 : 0;
  P.normals = c->have_normals ? 1 : 0;
}

// the two passes inside the producer frame; ksrc: the source slot, or -1 (the dense scalar src of type dt)
int derive_enqueue(smk_ctx *c, const char *who, const void *src, int dt, int ksrc, int step_out, int compat, int blur, hipStream_t s) {
  return smk_step_produce(c, who, step_out, ksrc, -1, s, [&](TimeStep &T, const TimeStep *S, const TimeStep *) -> int {
    DeriveParams P;
    derive_common(c, S ? S->vox : src, compat, blur, P);
    P.out = T.vox;
    P.st = (VghStats *)T.pass1_words;
    HIPCHK(c, S ? launch_derive_src<true>(c, P, c->dtype, PASS_1 | PASS_2, s) : launch_derive_src<false>(c, P, dt, PASS_1 | PASS_2, s));
    return 0;
  });
}

// ---------------------------------------------------------------------------------------------- the shard entries

constexpr int DV_REACH = 2;  // H reads the gradients of the neighbours, a blurred normal the differences of theirs: DV_AP

StencilEntry derive_shard_entry(const smk_ctx *c, const char *who) {
  StencilEntry E = derive_entry(c, who);
  E.sharded_why = "";
  return E;
}

DeriveShardParams derive_shard_params(const smk_ctx *c, const TimeStep &S, int compat, int blur) {
  DeriveShardParams P;
  derive_common(c, S.vox, compat, blur, P);
  smk_step_shard_box(c, S, DV_REACH, P.B);
  P.words_out = nullptr;
  P.words_in = nullptr;
  return P;
}

// ---------------------------------------------------------------------------------------------- the block entries

// the shard's parameters with the block as the source.  B: the region, and C shrunk by the reach as the result's valid box
DeriveBlockParams derive_block_params(const smk_ctx *c, const void *src, const smk_block *b, const SmkBlockView &V, int compat, int blur) {
  DeriveBlockParams P;
  derive_common(c, src, compat, blur, P);
  stencil_block_src(c, b, V, P);
  smk_step_block_box(c, V, DV_REACH, P.B);
  P.words_out = nullptr;
  P.words_in = nullptr;
  return P;
}

}  // namespace

int smk_derive_extremes_enqueue(smk_ctx *c, const char *who, int step_src, int compat, void *d_words, hipStream_t s) {
  int ksrc = -1;
  if (smk_step_shard_refusals(c, derive_shard_entry(c, who), DV_REACH, step_src, nullptr, &ksrc)) return 1;
  return smk_step_read(c, ksrc, -1, s, [&]() -> int {
    DeriveShardParams P = derive_shard_params(c, c->ts[(size_t)ksrc], compat, 0);
    P.words_out = (int *)d_words;
    HIPCHK(c, launch_derive_src<true>(c, P, c->dtype, PASS_1, s));
    return 0;
  });
}

extern "C" int smk_step_extremes_device(smk_ctx *c, int kind, int step_src, int compat, void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_step_extremes_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (stencil_kind_refusals(c, who, kind) || stencil_words_refusals(c, who, d_words)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return kind == SMK_EXTREMES_DERIVE ? smk_derive_extremes_enqueue(c, who, step_src, compat, d_words, s)
                                     : smk_merge_extremes_enqueue(c, who, step_src, d_words, s);
}

extern "C" int smk_block_extremes_device(smk_ctx *c, int kind, const void *const *d_fields, int nf, smk_dtype dtype, const smk_block *b,
                                         int compat, void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_block_extremes_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (stencil_kind_refusals(c, who, kind) || stencil_words_refusals(c, who, d_words)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (kind == SMK_EXTREMES_MERGE) return smk_merge_block_extremes_enqueue(c, who, d_fields, nf, dtype, b, d_words, s);
  SmkBlockView V;
  if (smk_step_block_refusals(c, derive_shard_entry(c, who), DV_REACH, nullptr, b, V)) return 1;
  if (!d_fields) FAIL(c, "%s: d_fields is NULL", who);
  if (nf != 1) FAIL(c, "%s: %d fields: the derive takes one scalar (nf 1)", who, nf);
  if (stencil_scalar_refusals(c, who, d_fields[0], dtype, -1, nullptr)) return 1;
  DeriveBlockParams P = derive_block_params(c, d_fields[0], b, V, compat, 0);
  P.words_out = (int *)d_words;
  HIPCHK(c, launch_derive_src<false>(c, P, dtype, PASS_1, s));
  return 0;
}

extern "C" int smk_upload_timestep_scalar_block_device(smk_ctx *c, int timestep, const void *d_scalar, smk_dtype scalar_dtype,
                                                       const smk_block *b, int compat, int blur, const void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_scalar_block_device";
  HIPCHK(c, hipSetDevice(c->device));
  SmkBlockView V;
  if (smk_step_block_refusals(c, derive_shard_entry(c, who), DV_REACH, &timestep, b, V)) return 1;
  if (stencil_scalar_refusals(c, who, d_scalar, scalar_dtype, timestep, nullptr) || stencil_words_refusals(c, who, d_words)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, timestep, -1, -1, s, [&](TimeStep &T, const TimeStep *, const TimeStep *) -> int {
    DeriveBlockParams P = derive_block_params(c, d_scalar, b, V, compat, blur);
    P.out = T.vox;
    P.words_in = (const int *)d_words;
    HIPCHK(c, launch_derive_src<false>(c, P, scalar_dtype, PASS_2, s));
    smk_step_block_done(c, V, DV_REACH, P.B, T);
    return 0;
  });
}

extern "C" int smk_derive_timestep_shard(smk_ctx *c, int step_src, int step_out, int compat, int blur, const void *d_words, void *stream) {
  if (!c) return 1;
  const char *who = "smk_derive_timestep_shard";
  HIPCHK(c, hipSetDevice(c->device));
  int ksrc = -1;
  if (smk_step_shard_refusals(c, derive_shard_entry(c, who), DV_REACH, step_src, &step_out, &ksrc)) return 1;
  if (stencil_words_refusals(c, who, d_words)) return 1;
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, step_out, ksrc, -1, s, [&](TimeStep &T, const TimeStep *S, const TimeStep *) -> int {
    DeriveShardParams P = derive_shard_params(c, *S, compat, blur);
    P.out = T.vox;
    P.words_in = (const int *)d_words;
    HIPCHK(c, launch_derive_src<true>(c, P, c->dtype, PASS_2, s));
    smk_step_shard_done(c, *S, DV_REACH, P.B, T);
    return 0;
  });
}

extern "C" int smk_derive_timestep(smk_ctx *c, int step_src, int step_out, int compat, int blur, void *stream) {
  if (!c) return 1;
  const char *who = "smk_derive_timestep";
  HIPCHK(c, hipSetDevice(c->device));
  int ksrc = -1;
  if (smk_step_stencil_refusals(c, derive_entry(c, who), step_out, &step_src, &ksrc)) return 1;
  return derive_enqueue(c, who, nullptr, c->dtype, ksrc, step_out, compat, blur, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_upload_timestep_scalar_device(smk_ctx *c, int timestep, const void *d_scalar, smk_dtype scalar_dtype, int sx, int sy,
                                                 int sz, int compat, int blur, void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_scalar_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (smk_step_stencil_refusals(c, derive_entry(c, who), timestep, nullptr, nullptr)) return 1;
  const int sizes[3] = {sx, sy, sz};
  if (stencil_scalar_refusals(c, who, d_scalar, scalar_dtype, timestep, sizes)) return 1;
  return derive_enqueue(c, who, d_scalar, (int)scalar_dtype, -1, timestep, compat, blur, stream ? (hipStream_t)stream : c->stream);
}
