// smk_slab.hip -- kernel S: the slice-ring ray-marcher (the fast path for 2-D / separable
// classification without perturbation or depth output).  DESIGN.md section 4 has the measurements
// behind every choice below.
//
// The gather kernel (smk_gather.hip) pulls 8 corners per sample through TA/L1: every 128-B line
// is re-requested from L2 several times and waves spend ~87 % of their time in s_waitcnt.  Here
// the volume is streamed instead:
//
//   * the principal axis S of the view (largest |ray direction| component in voxel space) is
//     chosen on the host; U is the memory-contiguous axis, V the third one (a lazily built
//     x-major copy of the volume serves S = x);
//   * a workgroup owns a pixel tile: NW consumer waves (one lane = one ray, a wave = a compact
//     8x8 sub-tile) plus NL loader waves;
//   * the loaders stream, front to back, the (u,v) window of every S-slice the tile's ray bundle
//     crosses from HBM straight into an LDS ring with LDS-DMA (global_load_lds_dwordx4, no VGPR
//     round trip): a lean issue loop (scalar address bumps, per-slice lane masks), a counted
//     s_waitcnt vmcnt(N) that retires the oldest slice in flight, a `landed` word per loader;
//   * every consumer wave advances on its own (no workgroup barrier in the main loop): one
//     sample per lane and iteration, taken when the two slices it touches have landed; the 8
//     corners come from LDS in one batch of reads behind one wait; the wave's progress (minimum
//     over its lanes) lets the loaders recycle ring slots;
//   * RGBA stays in registers front to back; 16 B per pixel leave the kernel.
//
// Each voxel row piece a tile needs is read once per tile; neighbouring tiles share the fringe
// (served by the XCD's L2: tiles are dealt to XCDs in contiguous, equal-work runs).
//
// Sample placement, membership and interpolation order are EXACTLY those of the gather kernel
// (same fma chains), so the two kernels agree bit for bit and the CPU checker on positions.
// Reference semantics: see smk_device.h.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <type_traits>

#include "smk_device.h"
#include "smk_slab.h"

#define SLAB_DONE 0x3fffffff
constexpr int SLAB_POLL_SLEEP = 2;  // s_sleep of a consumer wave between two polls for its next slices
// tools/slab_loop_isa.py --marks builds with -DSLAB_MARKS and cuts the consumer loop into its common and visible halves at
// these comments in the assembly.  Not in the product's build: an asm statement, even an empty one, holds code motion back,
// and on some instances that costs two or three VGPRs (profiles/r05_loop_diet.md)
#ifdef SLAB_MARKS
#define SLAB_MARK(what) asm volatile("; slab-mark: " what)
#else
#define SLAB_MARK(what) ((void)0)
#endif

template <int DT>
struct VoxT;
template <>
struct VoxT<0> {
  typedef uint2 type;
};
template <>
struct VoxT<1> {
  typedef float4 type;
};
template <>
struct VoxT<2> {  // u16 voxels (SMK_U16, smk.h): the u8 voxel's 8 bytes, staged and addressed the same way
  typedef uint2 type;
};

typedef float v2f __attribute__((ext_vector_type(2)));

// The 8 corners of one sample as ONE batch of LDS reads behind ONE wait.  Written as asm: left
// to hipcc the reads are either split into partial ds_read2_b32 pieces per use or (behind an
// optimisation barrier) waited for one by one -- 8 LDS round trips per sample.  a/b = byte
// addresses of corner (u,v) in the two slices, ap/bp = the same one row up; +VB = one voxel on.
// Only the channels classification needs are read here (2 or 3 floats / the 4 data bytes); the
// packed normals follow in a second batch for the samples that turn out to be visible: 16-24
// instead of 32 VGPRs live across the batch, and less LDS traffic for the transparent majority.
typedef float v3f __attribute__((ext_vector_type(3)));
#define SLAB_READ8(INS, OFF0, OFF1)                                                                                            \
  asm volatile(INS " %0, %8 offset:" OFF0 "\n\t" INS " %1, %8 offset:" OFF1 "\n\t" INS " %2, %9 offset:" OFF0 "\n\t"             \
               INS " %3, %9 offset:" OFF1 "\n\t" INS " %4, %10 offset:" OFF0 "\n\t" INS " %5, %10 offset:" OFF1 "\n\t"           \
               INS " %6, %11 offset:" OFF0 "\n\t" INS " %7, %11 offset:" OFF1 "\n\t"                                            \
               "s_waitcnt lgkmcnt(0)"                                                                                          \
               : "=&v"(q[0]), "=&v"(q[1]), "=&v"(q[2]), "=&v"(q[3]), "=&v"(q[4]), "=&v"(q[5]), "=&v"(q[6]), "=&v"(q[7])        \
               : "v"(a), "v"(ap), "v"(b), "v"(bp)                                                                              \
               : "memory")
// f32 voxels {c0, c1, c2, normal bits}: first two / three channels
__device__ __forceinline__ void slab_read8(unsigned a, unsigned ap, unsigned b, unsigned bp, v2f (&q)[8]) { SLAB_READ8("ds_read_b64", "0", "16"); }
__device__ __forceinline__ void slab_read8(unsigned a, unsigned ap, unsigned b, unsigned bp, v3f (&q)[8]) { SLAB_READ8("ds_read_b96", "0", "16"); }
// whole voxels (normals included) in one batch: workgroups that own a CU alone have the registers
// for it, and can then release their ring slots before classification and shading (EARLY below)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void slab_read8_full(unsigned a, unsigned ap, unsigned b, unsigned bp, v4f (&q)[8]) { SLAB_READ8("ds_read_b128", "0", "16"); }
__device__ __forceinline__ void slab_read8_full(unsigned a, unsigned ap, unsigned b, unsigned bp, v2u (&q)[8]) { SLAB_READ8("ds_read_b64", "0", "8"); }
// u8 voxels {4 data bytes, normal bits}: the data dword
__device__ __forceinline__ void slab_read8_u8(unsigned a, unsigned ap, unsigned b, unsigned bp, uint32_t (&q)[8]) { SLAB_READ8("ds_read_b32", "0", "8"); }
// the packed normals of the same 8 corners (dword NOFF of the voxel).  LEAN (the kernel's switch of that name): the dword's
// place in the voxel rides in the instruction's offset field, so the four corner addresses of the first batch serve every
// later one as they are -- four vector adds less per batch, and four addresses instead of two held across the visible path
template <bool LEAN>
__device__ __forceinline__ void slab_read8_nb16(unsigned a, unsigned ap, unsigned b, unsigned bp, uint32_t (&q)[8]) {
  if constexpr (LEAN) {
    SLAB_READ8("ds_read_b32", "12", "28");
  } else {
    a += 12; ap += 12; b += 12; bp += 12;
    SLAB_READ8("ds_read_b32", "0", "16");
  }
}
// the third float channel of the 8 corners (16-byte voxels), read on its own behind the (v, g) occupancy bit
template <bool LEAN>
__device__ __forceinline__ void slab_read8_h16(unsigned a, unsigned ap, unsigned b, unsigned bp, uint32_t (&q)[8]) {
  if constexpr (LEAN) {
    SLAB_READ8("ds_read_b32", "8", "24");
  } else {
    a += 8; ap += 8; b += 8; bp += 8;
    SLAB_READ8("ds_read_b32", "0", "16");
  }
}
template <bool LEAN>
__device__ __forceinline__ void slab_read8_nb8(unsigned a, unsigned ap, unsigned b, unsigned bp, uint32_t (&q)[8]) {
  if constexpr (LEAN) {
    SLAB_READ8("ds_read_b32", "4", "12");
  } else {
    a += 4; ap += 4; b += 4; bp += 4;
    SLAB_READ8("ds_read_b32", "0", "8");
  }
}
#undef SLAB_READ8

typedef __attribute__((address_space(3))) void *lds_ptr_t;
typedef __attribute__((address_space(3))) char *lds_cptr_w;
typedef const __attribute__((address_space(1))) void *glb_ptr_t;

// s_waitcnt vmcnt(n) for a wave-uniform runtime n (the instruction takes an immediate)
__device__ __forceinline__ void wait_vmcnt(int n) {
#define W(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    W(0) W(1) W(2) W(3) W(4) W(5) W(6) W(7) W(8) W(9) W(10) W(11) W(12) W(13) W(14) W(15)
    W(16) W(17) W(18) W(19) W(20) W(21) W(22) W(23) W(24) W(25) W(26) W(27) W(28) W(29) W(30) W(31)
    W(32) W(33) W(34) W(35) W(36) W(37) W(38) W(39) W(40) W(41) W(42) W(43) W(44) W(45) W(46) W(47)
    W(48) W(49) W(50) W(51) W(52) W(53) W(54) W(55) W(56) W(57) W(58) W(59) W(60) W(61) W(62) W(63)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef W
}

__device__ __forceinline__ int lds_ld(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_st(int *p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// LDS reads of the LOADER wave go through inline asm: with an LDS-DMA in flight hipcc puts
// s_waitcnt vmcnt(0) in front of every LDS read it can see (it cannot prove the read does not
// alias the DMA destination), which would drain the whole stream once per loop iteration.
// (cdna_hip_programming.md 5.7: the wait for an asm load is ours to place -- it is in the string.)
typedef __attribute__((address_space(3))) const void *lds_cptr_t;
__device__ __forceinline__ int raw_lds_b32(const void *p) {
  int v;
  unsigned a = (unsigned)(size_t)(lds_cptr_t)p;
  asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ uint2 raw_lds_b64(const void *p) {
  uint2 v;
  unsigned a = (unsigned)(size_t)(lds_cptr_t)p;
  asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
  return v;
}
__device__ __forceinline__ void raw_lds_st_b32(void *p, int v) {
  unsigned a = (unsigned)(size_t)(lds_cptr_t)p;
  asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory");
}

// minimum over the 64 lanes of a fully active wave, on the DPP network (no LDS traffic); the result is wave-uniform
// FOLD: the identity of min as the DPP move's `old` operand.  The compiler's DPP combiner then puts the modifier on the
// v_min_i32 itself -- with the value as `old` it cannot, and every step is v_mov + s_nop + v_mov_dpp + v_min -- and the rows
// are combined by row_bcast:15 / row_bcast:31 and ONE v_readlane of lane 63 instead of four v_readlane, an s_min, two v_mov
// and a v_min3: with the copy of the value that the caller goes on using, 8 vector issue slots instead of 20
// (tools/slab_loop_isa.py shows both).  Rows whose row_mask bit is clear keep their value: min(v, identity).  The plain
// frames' instances take it (TURN); the others keep the form their register allocation was settled with
template <bool FOLD>
__device__ __forceinline__ int wave_min_i32(int v) {
  if constexpr (FOLD) {
    constexpr int top = 0x7fffffff;
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x141, 0xf, 0xf, false));  // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x140, 0xf, 0xf, false));  // row_mirror
    // every row of 16 lanes now holds its own minimum
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x142, 0xa, 0xf, false));  // row_bcast:15: lane 15 of a row into the next, rows 1 and 3
    v = min(v, __builtin_amdgcn_update_dpp(top, v, 0x143, 0xc, 0xf, false));  // row_bcast:31: lane 31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);                                  // row 3 has seen all four
  } else {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));  // row_half_mirror
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));  // row_mirror
    // every row of 16 lanes now holds its own minimum
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
  }
}

// bilinear RGBA8 lookup like smk_tex2d, for tables of >= 2x2 texels: the clamped texel pair is
// always (i, i+1) then, so the four texels are two 8-byte loads at a 32-bit offset
struct SlabTexel4 {
  uint32_t a, b, c, d;
  float fs, ft;
};
template <bool LEAN>
__device__ __forceinline__ SlabTexel4 slab_tex2d_fetch(const uint32_t *tex, int ss, int s0, int t0, float fs, float ft) {
  SlabTexel4 o;
  o.fs = fs;
  o.ft = ft;
  // (LEAN: a 24-bit multiply, full rate -- a table has far fewer rows and columns; else the compiler's 64-bit multiply-add)
  const unsigned off = LEAN ? (__umul24((unsigned)t0, (unsigned)ss) + (unsigned)s0) * 4u : (unsigned)(t0 * ss + s0) * 4u;
  const char *tb = reinterpret_cast<const char *>(tex);
  uint2 lo, hi;
  __builtin_memcpy(&lo, tb + off, 8);
  __builtin_memcpy(&hi, tb + (off + (unsigned)ss * 4u), 8);
  o.a = lo.x;
  o.b = lo.y;
  o.c = hi.x;
  o.d = hi.y;
  return o;
}
__device__ __forceinline__ float slab_tex_chan(const SlabTexel4 &x, int k) {
  return smk_lerp(smk_lerp(smk_ub(x.a, k), smk_ub(x.b, k), x.fs), smk_lerp(smk_ub(x.c, k), smk_ub(x.d, k), x.fs), x.ft) * SMK_INV255;
}

// NW = consumer waves (64 rays each), NL = loader waves; the block has (NW+NL)*64 threads, the
// last NL waves are loaders: loader l streams DMA chunks l, l+NL, ... of every slice.
// second launch-bound = waves per SIMD wanted: workgroups of 5/9/10 waves only double up on a CU
// (2 x 9 waves = 5 on one SIMD) if the kernel stays within 96 VGPRs
// TF: 1 = 2-D (V,G) table x optional third-axis alpha (NV20VolRen3D.cpp:544-596), 2 = dense 3-D (v,g,h)
// table (TFWidgetRen.cpp:779-845; BASELINE configs 4/5)
// (BR: the instance knows about brick flags -- EMPTY LAYERS; frames without flags run instances that carry none of it:
//  the run-time test alone, three per loop turn, cost them 12 % in scalar registers spilled)
// (SHD: the frame's planes are the half-angle slices of a frame with shadows -- SmkShadowRays; the eye pass of smk_shadow.hip.
//  Compile-time: the instances live in SLAB_PART 2 and 7)
// (OCC: the frame has the host's opaque scene depth, smk_render_occluded -- folded into each ray's plane range in the set-up.
//  Compile-time as well: as a run-time test it cost the instances of frames without one a VGPR and a few SGPR spills; the
//  instances live in SLAB_PART 3 and 4)
// (NVL: the NV20 look of a frame with shadows, option shadow_look 1 -- the sample keeps 1 - sat(light-buffer opacity) (1 - amb)
//  of its colour, smk_shadow_keep.  Compile-time as SHD is, SHD instances without OCC only: SLAB_PART 5)
template <int DT, int SH, int PERM, int NW, int NL, bool DIAG, int TF = 1, bool BR = true, bool SHD = false, bool OCC = false, bool NVL = false>
// (second argument: waves per SIMD the register allocation must allow -- two small workgroups per CU)
__global__ __launch_bounds__((NW + NL) * 64, ((NW + NL) == 9) ? 6 : ((NW + NL) == 5 || (NW + NL) == 10) ? 5 : ((NW + NL) == 11 ? 3 : (NW + NL) == 12 ? 6 : 4)) void smk_k_slab(const RenderParams P, const SlabParams Q) {
  constexpr int UPV = DT != 1 ? 2 : 1;   // voxels per 16-byte DMA unit (by voxel size: u8 and u16 voxels are 8 bytes)
  constexpr int VB = DT != 1 ? 8 : 16;   // bytes per voxel
  // (global_load_lds_dwordx3 does NOT compact: it writes 12 bytes per lane at a 16-byte lane stride
  //  -- tools/dma_layout_probe.hip -- so staging only {c0,c1,c2} needs a 12-byte HBM plane)
  constexpr int VBL = DT != 1 ? 3 : 4;   // log2
  constexpr int NTH = (NW + NL) * 64;
  // big workgroups (one per CU, 128 VGPRs each): read whole voxels, release ring slots early
  // (re-measured with the loaders in pairs: without the early release 4.56 vs 4.11 ms on the 1024^3 frame)
  constexpr bool BIG = slab_big(NW, NL);
  constexpr bool EARLY = BIG;
  // LEAN: the shorter instruction stream of a consumer's turn (*Instruction stream of a turn*) -- the
  // slice-table entry by one multiply-add, later batches of corner reads through the first batch's addresses, the texel
  // offset by a 24-bit multiply.  The same operations on the same values, but another register allocation: the plain frames'
  // instances have the room, those of frames with shadows, scene depth or the NV20 look sit at the 80 VGPRs of their launch
  // bound and would pass it or need scratch (profiles/r05_loop_diet.md), so they keep the longer form
  constexpr bool LEAN = !SHD && !OCC && !NVL;
  // TURN: the compiler's bookkeeping taken out of a turn (same section, second part) -- the wave minimum with the DPP modifier
  // folded into v_min_i32, `work` as a lane mask, one nested visible block.  The diagnostic instances keep the older forms:
  // with their counters and time stamps they hold more live values, and the 10+2 ones gained 4 bytes of scratch with the new
  constexpr bool TURN = LEAN && !DIAG;
  static_assert(VB % 8 == 0, "TURN reads the low bits of a slice-table entry as flags: bases must be multiples of 8");
  // ... and their loaders skip the row groups a slice does not need, counting DMA instructions per
  // slice; small workgroups keep every slice the same number of instructions (cheaper bookkeeping:
  // measured 3 % on the 512^3 frame, where the loaders' issue slots are the consumers')
  constexpr bool FIFO = BIG;
  // Small workgroups: the loaders take WHOLE slices in turn (loader l streams slices l, l + NL, ...) instead of a share of
  // the row groups of every slice.  A slice costs a loader ~120 scalar instructions before its first DMA (ring check,
  // table entry, 64-bit source address, column masks); with 3 DMA instructions per loader and slice that overhead was the
  // larger part of the loaders' time, and they were busy 90 % of the frame.  Big workgroups keep the split: their ring is
  // too short for NL slices being filled at once.
  // Generalised: the loaders form NLG groups of LPG loaders each (slab_loader_groups, smk_slab.h).
  constexpr int NLG = slab_loader_groups(NW, NL);
  constexpr int LPG = NL / NLG;
  constexpr int QSTEP = NLG;
  extern __shared__ __align__(16) unsigned char smem[];
  // LDS carve: ring [nslots][slot_bytes] | slice table [Ds] | control words | alpha_H
  SlabEnt *wtab = reinterpret_cast<SlabEnt *>(smem + (size_t)Q.nslots * Q.slot_bytes);
  // control words: [0] smin [1] smax [3] error flag [4..4+NL) landed per loader [8..8+NW) progress
  int *ctl = reinterpret_cast<int *>(smem + (((size_t)Q.nslots * Q.slot_bytes + (size_t)Q.Ds * sizeof(SlabEnt) + 15) & ~(size_t)15));
  // third-axis alpha as a 1-D table: with <= 3 channels the (H,4th) lookup has t = 0, i.e. row
  // 0 of deptex2 with a zero t-weight, so lerp(row0[s0], row0[s1], fs) is the SAME float
  float *ah = reinterpret_cast<float *>(ctl + 8 + 32);
  // occupancy bitmap of the (V,G) table (smk_api.hip refresh_tf2d), a copy per workgroup
  const uint32_t *occ = reinterpret_cast<const uint32_t *>(ah + (Q.use_ah ? P.sv : 0));

  // order entry: tile | segment << 20 | segments of the tile << 26 (DEPTH SEGMENTS below); -1 = none
  const int2 oent = Q.order[blockIdx.x];
  const int ocode = oent.x;
  if (ocode < 0) return;  // whole workgroup leaves together
  const int tile = ocode & 0xfffff, seg = (ocode >> 20) & 63, nseg = max((ocode >> 26) & 31, 1);
  const int cut_lo = oent.y & 255, cut_hi = (oent.y >> 8) & 255;  // this piece's share of the tile's slice positions, in 255ths
  const bool flags = BR && Q.bricks != nullptr;
  const bool tracing = DIAG && Q.trace != nullptr && (P.lockstep & 32);  // (diagnostic: workgroup timeline)
  // the workgroup's duration feeds the next frame's schedule (see slab_measured_weights in smk_slab_plan.hip): one scalar
  // timestamp at each end and one 4-byte store per tile
  const unsigned trace_t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
  const int ty = tile / P.ntx, tx = tile - ty * P.ntx;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: roles and loops stay wave-uniform
  const bool is_loader = wave >= NW;
  const int lid = wave - NW;  // loader index
  // consumer wave = 8x8 pixel sub-tile; waves laid out row-major over the tile
  const int wpr = Q.tw >> 3;
  const int i = tx * Q.tw + (wave % wpr) * 8 + (lane & 7);
  const int j = ty * Q.th + (wave / wpr) * 8 + (lane >> 3);
  const bool live = !is_loader && i < P.W && j < P.H;

  const smk_raycoef &rc = P.rc;
  const float px = __fmaf_rn((float)i + 0.5f, rc.pxs, rc.pxl);
  const float py = __fmaf_rn((float)j + 0.5f, rc.pys, rc.pyl);
  float A[3], B[3], tauA, dtau;  // (tauA, dtau: frames with shadows only -- the ray parameter of plane q is fma(q, dtau, tauA), smk_ray_AB)
  const bool ray_ok = smk_ray_AB_t<SHD>(P, px, py, A, B, tauA, dtau);
  // conservative plane range (identical to the gather kernel)
  float tenter = 0.0f, texit = (float)(rc.nplanes - 1);
  bool empty = rc.nplanes <= 0 || !live || !ray_ok;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (fabsf(B[a]) > 1e-20f) {
      float inv = 1.0f / B[a];
      // (the box is widened by SMK_RANGE_EPS voxels: a ray that runs ALONG a face -- the centre row of an odd
      //  viewport along a shard boundary -- has fma(m, B, A) round onto the face for every m although
      //  (lo - A) / B says it leaves at m = 0; the exact per-sample test decides, this only brackets it)
      float t1 = (P.lo[a] - SMK_RANGE_EPS - A[a]) * inv, t2 = (P.hi[a] + SMK_RANGE_EPS - A[a]) * inv;
      tenter = fmaxf(tenter, fminf(t1, t2) - 2.0f);
      texit = fminf(texit, fmaxf(t1, t2) + 2.0f);
    } else if (!(A[a] >= P.lo[a] && A[a] <= P.hi[a])) {
      empty = true;
    }
  }
  // Free clip plane (glClipPlane, NV20VolRen3D.cpp:346-357): fragments on its negative side do not exist.  The plane's value
  // along a ray, cplane . (p(q), 1), is monotone in the plane index q like the coordinates: the kept samples are an interval
  // that ends where it crosses zero -- folded into the ray's range HERE, the marching loop never hears of it (as a test per
  // sample in the loop it cost every frame without a clip plane 4-5 %: round 2).
  if (P.cplane_on) {
    const float c0 = __fmaf_rn(A[0], P.cplane[0], __fmaf_rn(A[1], P.cplane[1], __fmaf_rn(A[2], P.cplane[2], P.cplane[3])));
    const float c1 = __fmaf_rn(B[0], P.cplane[0], __fmaf_rn(B[1], P.cplane[1], B[2] * P.cplane[2]));
    if (fabsf(c1) > 1e-20f) {
      const float tz = -c0 / c1;  // the crossing, in planes
      if (c1 > 0.0f) tenter = fmaxf(tenter, tz - 2.0f);
      else texit = fminf(texit, tz + 2.0f);
    } else if (!(c0 >= 0.0f)) {
      empty = true;
    }
  }
  // Frames with shadows: a sample exists where its ray parameter fma(q, dtau, tauA) is positive -- monotone in q like the clip
  // plane's value, folded into the range the same way.
  if (SHD && ray_ok) {
    if (fabsf(dtau) > 1e-30f) {
      const float tz = -tauA / dtau;
      if (dtau > 0.0f) tenter = fmaxf(tenter, tz - 2.0f);
      else texit = fminf(texit, tz + 2.0f);
    } else if (!(tauA > 0.0f)) {
      empty = true;
    }
  }
  // The host's opaque scene depth (smk_render_occluded): a sample exists where its smk_plane_depth is below the pixel's --
  // monotone in q as well (smk_scene_bracket), folded the same way and tested exactly at the ends by inside() below.
  float zD = __int_as_float(0x7f800000);
  if (OCC && live) {
    zD = smk_scene_depth(P, (size_t)j * P.W + i);
    smk_scene_bracket(zD, SHD ? tauA : rc.tau0, SHD ? dtau : rc.dtau, P.znear, tenter, texit, empty);
  }
  int m = (int)floorf(fmaxf(tenter, 0.0f));
  int m1 = (int)ceilf(fminf(texit, (float)(rc.nplanes - 1)));
  if (empty || !(tenter <= texit)) m1 = m - 1;
  // Exact first/last inside sample.  A coordinate fma(q, B, A) is monotone in q (one correctly
  // rounded operation), so the samples that pass the membership predicate of the gather kernel
  // -- lo <= p <= hin on every axis, hin = hi itself on a top face, else the float just below
  // it -- form ONE interval of q; the conservative range above brackets it with a few planes of
  // slack, so testing its ends here removes the per-sample test from the marching loop.
  {
    auto inside = [&](int q) -> bool {
      const float qf = (float)q;
      const float p0 = __fmaf_rn(qf, B[0], A[0]), p1 = __fmaf_rn(qf, B[1], A[1]), p2 = __fmaf_rn(qf, B[2], A[2]);
      bool in = ((int)(smk_clampf(p0, P.lo[0], P.hin[0]) == p0) & (int)(smk_clampf(p1, P.lo[1], P.hin[1]) == p1) &
                 (int)(smk_clampf(p2, P.lo[2], P.hin[2]) == p2)) != 0;
      // (the gather kernel's own fma chain for the plane: the same samples pass, bit for bit)
      if (P.cplane_on) in = in && __fmaf_rn(p0, P.cplane[0], __fmaf_rn(p1, P.cplane[1], __fmaf_rn(p2, P.cplane[2], P.cplane[3]))) >= 0.0f;
      if (SHD) in = in && smk_tau_ok(tauA, dtau, q);
      if constexpr (OCC) in = in && smk_plane_depth<SHD>(P, q, tauA, dtau) < zD;  // (depth_out's chain: the same bits)
      return in;
    };
    int mf = m1 + 1, ml = m - 1;
    int qa = m, qb = m1;
    // (the ends move inwards until they are inside; rays that only graze the region end empty)
    while (true) {
      const bool go_a = qa <= m1 && mf > m1, go_b = qb >= m && ml < m;
      if (!__any(go_a || go_b)) break;  // (a few steps: the slack is +-2 planes)
      if (go_a) {
        if (inside(qa)) mf = qa;
        ++qa;
      }
      if (go_b) {
        if (inside(qb)) ml = qb;
        --qb;
      }
    }
    m = mf;  // (no inside sample at all: mf = m1 + 1 > ml, the ray is empty)
    m1 = ml;
  }

  constexpr int AS = PERM == 0 ? 2 : (PERM == 1 ? 1 : 0);
  constexpr int AU = PERM == 2 ? 1 : 0;
  constexpr int AV = PERM == 0 ? 1 : 2;
  const int NS = P.N[AS], NU = P.N[AU], NV = P.N[AV];

  // base slice index of plane q on this ray (a sample reads slices i0 and i0+1)
  auto base_slice = [&](int q) -> int {
    float s = __fmaf_rn((float)q, B[AS], A[AS]);
    float sc = smk_clampf(s, 0.0f, (float)(NS - 1));
    return min((int)sc, NS - 2);
  };
  // the same, also handing out the clamped coordinate: exactly smk_lin_clamp's (xc, i0) of the principal axis, which the
  // sample of plane q needs again one loop turn later (carried instead of recomputed: 4 VALU per turn; within noise on both frames)
  auto base_slice_c = [&](int q, float &sc_out) -> int {
    float s = __fmaf_rn((float)q, B[AS], A[AS]);
    sc_out = smk_clampf(s, 0.0f, (float)(NS - 1));
    return min((int)sc_out, NS - 2);
  };
  float car_sc = 0.f;  // clamped principal-axis coordinate and base slice of THIS ray's next sample (plane m)
  int car_i = 0;

  // ---- workgroup slice range
  if (tid == 0) {
    ctl[0] = 0x7fffffff;
    ctl[1] = -0x7fffffff;
    ctl[2] = 0;  // slices the loaders did not have to stream (EMPTY LAYERS)
    ctl[3] = 0;  // error flag (bounded spins, window bound)
    for (int l = 0; l < 4; ++l) ctl[4 + l] = l < NL ? l % NLG : 0x7fffffff;  // (a loader's first slice) absent loaders never hold anyone back
  }
  if (tid < 32) ctl[8 + tid] = (NL > 4 && tid >= 16 && tid < 12 + NL) ? (tid - 12) % NLG : SLAB_DONE;  // (ctl[24..27]: loaders 4..7)
  __syncthreads();
  {
    int lo = 0x7fffffff, hi = -0x7fffffff;
    if (m <= m1) {
      int a0 = base_slice(m), a1 = base_slice(m1);
      lo = min(a0, a1);
      hi = max(a0, a1);
    }
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, __shfl_xor(lo, o));
      hi = max(hi, __shfl_xor(hi, o));
    }
    if (lane == 0 && lo <= hi) {
      atomicMin(&ctl[0], lo);
      atomicMax(&ctl[1], hi);
    }
  }
  __syncthreads();
  int smin = ctl[0], smax = ctl[1];
  // ---- DEPTH SEGMENTS.  A tile whose workgroup would run long (measured, see the launcher) is rendered by `nseg`
  // workgroups: the positions of its slice range are cut into nseg runs (where, the launcher decides from the pieces'
  // measured durations: equal WORK, not equal depth), workgroup `seg` takes the samples whose base
  // slice lies in its run -- base slices are monotone in the plane index, so a ray's share is a sub-interval of its
  // planes, found by an estimate and the exact evaluation -- and writes a partial frame; the partial frames are merged
  // in marching order afterwards (smk_k_slab_merge: front-to-back over, or max).  What changes is the association of
  // the blend, nothing else: the frame agrees with the unsplit one to a few ulp per segment.
  if (nseg > 1 && smin <= smax) {
    const int np_full = smax - smin + 1;
    const int q0 = (int)((long long)cut_lo * np_full / 255), q1 = (int)((long long)cut_hi * np_full / 255);  // positions [q0, q1)
    // base slices of this segment
    const int b_lo = Q.dir > 0 ? smin + q0 : smax - q1 + 1, b_hi = Q.dir > 0 ? smin + q1 - 1 : smax - q0;
    if (m <= m1) {
      if (q1 <= q0) {
        m1 = m - 1;
      } else {
        const float inv = 1.0f / B[AS];
        // first plane whose base slice is inside [b_lo, b_hi] in marching order: s reaches the run's near face
        const float s_near = Q.dir > 0 ? (float)b_lo : (float)(b_hi + 1), s_far = Q.dir > 0 ? (float)(b_hi + 1) : (float)b_lo;
        auto in_run = [&](int q) -> bool { const int b = base_slice(q); return b >= b_lo && b <= b_hi; };
        auto before = [&](int q) -> bool { const int b = base_slice(q); return Q.dir > 0 ? b < b_lo : b > b_hi; };
        // (at an end of the volume the clamped base slice takes in everything beyond: no estimate, the ray's own end)
        const bool open_near = Q.dir > 0 ? b_lo <= 0 : b_hi >= NS - 2, open_far = Q.dir > 0 ? b_hi >= NS - 2 : b_lo <= 0;
        int qa = open_near ? m : max(m, min(m1 + 1, (int)floorf((s_near - A[AS]) * inv) - 1));
        int qb = open_far ? m1 : min(m1, max(m - 1, (int)ceilf((s_far - A[AS]) * inv) + 1));
        bool bad = false;
#pragma unroll 1
        for (int k = 0; qa <= m1 && before(qa); ++k) { ++qa; if (k > 8) { bad = true; break; } }   // up to the run
#pragma unroll 1
        for (int k = 0; qa > m && !before(qa - 1); ++k) { --qa; if (k > 8) { bad = true; break; } }  // (never started inside it)
#pragma unroll 1
        for (int k = 0; qb >= qa && !in_run(qb) && !before(qb); ++k) { --qb; if (k > 8) { bad = true; break; } }  // back into the run
#pragma unroll 1
        for (int k = 0; qb < m1 && (in_run(qb + 1) || before(qb + 1)); ++k) { ++qb; if (k > 8) { bad = true; break; } }
        if (bad) ctl[3] = 1;  // the bracket did not close: reported, the frame is rendered again another way
        m = qa;
        m1 = (qb >= qa && in_run(qb) && in_run(qa)) ? qb : qa - 1;
      }
    }
    smin = b_lo;
    smax = b_hi;
    if (q1 <= q0) { smin = 0x7fffffff; smax = -0x7fffffff; }
  }
  const bool phases = tracing && (P.lockstep & 128);  // (diagnostic: where the set-up's time goes, instead of the loader's cycles)
  unsigned ph1 = 0, ph2 = 0, ph3 = 0;
  if (phases) ph1 = (unsigned)__builtin_amdgcn_s_memrealtime() - trace_t0;
  const int dir = Q.dir, nslots = Q.nslots;
  // LDS row pitch in bytes (LEAN: the mask says what the host guarantees -- the 24-bit multiplies of the loop then take this
  // very register and not a masked copy of it)
  const unsigned pitch_b = LEAN ? (16u * (unsigned)Q.wp) & 0xffffffu : 16u * (unsigned)Q.wp;
  const unsigned ring_addr = (unsigned)(size_t)(lds_cptr_t)smem;
  // positions p = 0..npos-1 in marching order: base slice b(p) = dir>0 ? smin+p : smax-p;
  // load order q = 0..npos: slice L(q) = dir>0 ? smin+q : smax+1-q; position p reads L(p), L(p+1)
  const int npos = smax - smin + 1;
  // ---- per-slice windows of this tile (every thread fills some table entries).  Every window
  // has the SAME shape (Q.wu units x Q.wv rows, host-sized to cover the widest bundle section)
  // so a DMA lane's source offset inside the window never changes; only its origin moves: the
  // bbox, over the tile's 4 corner rays, of every position a sample touching slice sl can have
  // (s in [sl-1, sl+1], stretched to the volume faces at the ends)
  if (npos > 0) {
    float cA[4][3], cB[4][3];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int ci = min(tx * Q.tw + ((c & 1) ? Q.tw - 1 : 0), P.W - 1);
      int cj = min(ty * Q.th + ((c & 2) ? Q.th - 1 : 0), P.H - 1);
      float cx = __fmaf_rn((float)ci + 0.5f, rc.pxs, rc.pxl), cy = __fmaf_rn((float)cj + 0.5f, rc.pys, rc.pyl);
      float cta, cdt;
      (void)smk_ray_AB_t<SHD>(P, cx, cy, cA[c], cB[c], cta, cdt);  // (the launcher declines frames whose rays can run parallel to the slices)
    }
    if (Q.use_ah)
      for (int e = tid; e < P.sv; e += NTH) ah[e] = smk_ub(P.tf_h[e], 3);
    if (Q.use_occ) {
      uint32_t *occ_w = const_cast<uint32_t *>(occ);
      for (int e = tid; e < P.occ_roww * (TF == 2 ? P.s3g : P.sg); e += NTH) occ_w[e] = P.tf_occ[e];
    }
    const int wuv = Q.wu * UPV;  // window width in voxels
    for (int q = tid; q <= npos; q += NTH) {
      int sl = dir > 0 ? smin + q : smax + 1 - q;  // global slice index
      int e = sl - Q.Os;
      if (e < 0 || e >= Q.Ds) continue;
      float s_lo = sl <= 1 ? -0.5f : (float)(sl - 1), s_hi = sl >= NS - 2 ? (float)NS - 0.5f : (float)(sl + 1);
      float umin = 1e30f, umax = -1e30f, vmin = 1e30f, vmax = -1e30f;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float ib = 1.0f / cB[c][AS];
        float ma = (s_lo - cA[c][AS]) * ib, mb = (s_hi - cA[c][AS]) * ib;
        float ua = __fmaf_rn(ma, cB[c][AU], cA[c][AU]), ub = __fmaf_rn(mb, cB[c][AU], cA[c][AU]);
        float va = __fmaf_rn(ma, cB[c][AV], cA[c][AV]), vb = __fmaf_rn(mb, cB[c][AV], cA[c][AV]);
        umin = fminf(umin, fminf(ua, ub));
        umax = fmaxf(umax, fmaxf(ua, ub));
        vmin = fminf(vmin, fminf(va, vb));
        vmax = fmaxf(vmax, fmaxf(va, vb));
      }
      // texel pair of coordinate x is floor(clamp(x)), +1; SLAB_EPS absorbs fp differences
      // between this bbox and the per-sample chains
      int u0 = (int)floorf(fminf(fmaxf(umin - SLAB_EPS, 0.0f), (float)(NU - 2)));
      int u1 = (int)floorf(fminf(fmaxf(umax + SLAB_EPS, 0.0f), (float)(NU - 2))) + 1;
      int v0 = (int)floorf(fminf(fmaxf(vmin - SLAB_EPS, 0.0f), (float)(NV - 2)));
      int v1 = (int)floorf(fminf(fmaxf(vmax + SLAB_EPS, 0.0f), (float)(NV - 2))) + 1;
      // to stored-box coordinates, clipped to it
      u0 = max(u0 - Q.Ou, 0);
      v0 = max(v0 - Q.Ov, 0);
      u1 = min(u1 - Q.Ou, Q.Du - 1);
      v1 = min(v1 - Q.Ov, Q.Dv - 1);
      if (UPV == 2) u0 &= ~1;  // rows start on whole 16-byte units (the stored U extent is even)
      // fixed-shape window: slide it back inside the stored box where it would stick out
      const int wu0 = min(u0, Q.Du - wuv), wv0 = min(v0, Q.Dv - Q.wv);
      if (u1 - wu0 + 1 > wuv || v1 - wv0 + 1 > Q.wv) ctl[3] = 2;  // host bound violated: reported, never silent
      // what this slice really needs of the fixed-shape window (the loader masks the rest)
      const int need_u = max((u1 - wu0 + UPV) / UPV, 1), need_v = max(v1 - wv0 + 1, 1);
      SlabEnt ent;
      ent.pack = (unsigned)wu0 | ((unsigned)wv0 << 11) | ((unsigned)(min(need_u, Q.wu) - 1) << 22) |
                 ((unsigned)min(15, max(Q.wv - need_v, 0) / ((Q.wv + 15) / 16)) << 28);  // rows spared, in 1/16ths of wv (rounded down)
      ent.base = (int)ring_addr + (q % nslots) * Q.slot_bytes - (Q.Ov + wv0) * (int)pitch_b - (Q.Ou + wu0) * VB;
      wtab[e] = ent;
    }
  }
  if (phases) {
    __syncthreads();
    ph2 = (unsigned)__builtin_amdgcn_s_memrealtime() - trace_t0;
  }
  // ---- EMPTY LAYERS.  The cells between slices b and b + 1 ("layer b") that this tile's rays can cross lie in the
  // overlap of the two slices' windows.  When every brick that overlap touches is flagged empty (smk_bricks.hip: no
  // sample in it can be visible under the current table), nobody in the tile samples layer b -- bit 0 of the entry --
  // and a slice whose two neighbouring layers are both empty is not streamed at all -- bit 1.  (The entries' base
  // addresses are multiples of 8.)  A sample that IS taken therefore finds both its slices loaded: its layer's bit 0 is
  // clear, which keeps bit 1 of both slices clear.  An entry whose slice is not streamed needs no address: it holds,
  // above the two bits, how many empty layers follow one another from this one on in marching order (to the end of
  // the tile's range = "the rest"); rays and loaders step over such a run at once (see there).
  // Three steps, a barrier between them; the flags are read from memory once per layer of BRICKS, a lane per brick:
  // (the first version read them per slice and thread, one after the other: 40 us per workgroup, a fifth of the frame)
  if (flags && npos > 0) {
    constexpr int BL = SMK_BRICK_LOG2;
    __syncthreads();
    auto extent = [&](int e, int &ulo, int &uhi, int &vlo, int &vhi) {
      const unsigned pk = wtab[e].pack;
      ulo = (int)(pk & 0x7ffu);
      vlo = (int)((pk >> 11) & 0x7ffu);
      uhi = ulo + (int)(((pk >> 22) & 0x3fu) + 1u) * UPV - 1;
      vhi = vlo + (Q.wv - (int)(pk >> 28) * ((Q.wv + 15) / 16)) - 1;
    };
    // (1) per layer of bricks along S: origin (first brick the tile's windows touch there) and the flags of the 8 x 8
    // bricks from it on, as a 64-bit mask -- kept in the ring's memory, which nobody uses before the last barrier
    uint4 *lmask = reinterpret_cast<uint4 *>(smem);
    const int nlay = ((Q.Ds - 1) >> BL) + 1;
    // (eight layers per wave and round, so that a workgroup's loads are all in flight at once: lane 8 k + j reads the
    //  window origin of slice j of layer k, the eight lanes of a group reduce to the layer's origin; two rounds of four
    //  layers with every lane looping over the entries took 9-10 us of the set-up's 19)
    static_assert(SMK_BRICK_LOG2 == 3, "the lane mapping below assumes eight slices per layer of bricks");
    for (int bl0 = wave * 8; bl0 < nlay; bl0 += (NW + NL) * 8) {
      int ulo = 0x7fffffff, vlo = 0x7fffffff;
      {
        const int e = ((bl0 + (lane >> 3)) << BL) + (lane & 7);
        const int sl = e + Q.Os;
        if (e < Q.Ds && sl >= smin && sl <= smax + 1) {
          const unsigned pk = wtab[e].pack;
          ulo = (int)(pk & 0x7ffu);
          vlo = (int)((pk >> 11) & 0x7ffu);
        }
      }
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        ulo = min(ulo, __shfl_xor(ulo, o));
        vlo = min(vlo, __shfl_xor(vlo, o));
      }
      int bu0[8], bv0[8];
      unsigned f[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int lu = __builtin_amdgcn_readlane(ulo, k * 8), lv = __builtin_amdgcn_readlane(vlo, k * 8);
        bu0[k] = lu >> BL;
        bv0[k] = lv >> BL;
        f[k] = 0;
        const int bu = bu0[k] + (lane & 7), bv = bv0[k] + (lane >> 3);
        if (bl0 + k < nlay && lu != 0x7fffffff && bu <= ((Q.Du - 1) >> BL) && bv <= ((Q.Dv - 1) >> BL))
          f[k] = Q.bricks[(size_t)(bl0 + k) * Q.bss + (size_t)bv * Q.bsv + (size_t)bu * Q.bsu];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const unsigned long long m = __ballot(f[k] != 0);
        if (lane == 0 && bl0 + k < nlay) lmask[bl0 + k] = make_uint4((unsigned)bu0[k], (unsigned)bv0[k], (unsigned)m, (unsigned)(m >> 32));
      }
    }
    __syncthreads();
    // (2) per slice: is its layer empty for this tile (bit 0), does anybody need the slice (bit 1)
    auto layer_empty = [&](int sl) -> bool {  // layer sl, smin <= sl <= smax
      const int e = sl - Q.Os;
      int ulo, uhi, vlo, vhi;
      extent(e, ulo, uhi, vlo, vhi);
      if (e + 1 < Q.Ds) {  // (slice sl + 1 <= smax + 1 is in the tile's range: its entry is filled)
        int u2, u3, v2, v3;
        extent(e + 1, u2, u3, v2, v3);
        ulo = max(ulo, u2);
        uhi = min(uhi, u3);
        vlo = max(vlo, v2);
        vhi = min(vhi, v3);
      }
      // lower corners of the cells: one less than the voxels at the top end
      uhi = min(uhi, Q.Du - 1) - 1;
      vhi = min(vhi, Q.Dv - 1) - 1;
      if (uhi < ulo || vhi < vlo) return true;
      const uint4 L = lmask[e >> BL];
      const int c0 = (ulo >> BL) - (int)L.x, c1 = (uhi >> BL) - (int)L.x, r0 = (vlo >> BL) - (int)L.y, r1 = (vhi >> BL) - (int)L.y;
      if (c0 < 0 || r0 < 0 || c1 > 7 || r1 > 7) return false;  // (outside the square that was looked at: not known to be empty)
      const unsigned long long cols = (unsigned long long)((0xffu >> (7 - c1)) & (0xffu << c0)) * 0x0101010101010101ull;
      const unsigned long long rows = (~0ull >> (8 * (7 - r1))) & (~0ull << (8 * r0));
      const unsigned long long m = (unsigned long long)L.z | ((unsigned long long)L.w << 32);
      return (m & cols & rows) == 0;
    };
    for (int q = tid; q <= npos; q += NTH) {
      const int sl = dir > 0 ? smin + q : smax + 1 - q;
      const int e = sl - Q.Os;
      if (e < 0 || e >= Q.Ds) continue;
      const bool mine = sl <= smax && !layer_empty(sl);
      const bool below = sl - 1 >= smin && e - 1 >= 0 && !layer_empty(sl - 1);
      int fl = mine ? 0 : 1;
      if (!mine && !below) fl |= 2;
      if (fl) wtab[e].base |= fl;
    }
    __syncthreads();
    // (3) run lengths, by one wave: 64 positions at a time from the far end, a ballot each (the run that starts at a
    // position = the trailing ones of the mask from its bit on, + the next block's first run when it reaches the end)
    if (wave == 0) {
      int carry = 0x40000;  // behind the last position: "the rest"
      for (int blk = (npos - 1) >> 6; blk >= 0; --blk) {
        const int pq = (blk << 6) + lane;                  // position in marching order
        const int sl = dir > 0 ? smin + pq : smax - pq;    // its layer
        const int e = sl - Q.Os;
        int bits = 3;                                      // (behind the range: counts as empty)
        if (pq < npos) bits = (e >= 0 && e < Q.Ds) ? (wtab[e].base & 3) : 0;
        const unsigned long long m = __ballot((bits & 1) != 0);
        const unsigned long long rest = ~(m >> lane);      // (the shift brings in zeros: the count stops at the block's end)
        int run = rest ? (int)__builtin_ctzll(rest) : 64;
        if (run == 64 - lane) run += carry;
        if (pq < npos && bits == 3) wtab[e].base = (min(run, 0x7ffff) << 2) | 3;
        carry = __builtin_amdgcn_readlane(run, 0);
      }
      if (lane == 0) {  // the slice behind the last layer (no layer of its own)
        const int e = smax + 1 - Q.Os;
        if (e >= 0 && e < Q.Ds && (wtab[e].base & 3) == 3) wtab[e].base = (1 << 2) | 3;
      }
    }
  }
  // every consumer wave announces the first position it needs before anyone moves on
  const int psgn = dir > 0 ? 1 : -1, poff = dir > 0 ? -smin : smax;  // position of base slice b = psgn*b + poff
  int pb = SLAB_DONE;  // position of this ray's next sample
  if (m <= m1) {
    car_i = base_slice_c(m, car_sc);
    pb = psgn * car_i + poff;
  }
  int pos = SLAB_DONE;
  if (!is_loader && npos > 0) {
    pos = wave_min_i32<TURN>(pb);
    if (lane == 0) ctl[8 + wave] = pos;
  }
  __syncthreads();  // table, alpha_H, control words visible; LAST workgroup barrier
  if (phases) ph3 = (unsigned)__builtin_amdgcn_s_memrealtime() - trace_t0;
  float C0 = 0.f, C1 = 0.f, C2 = 0.f, C3 = 0.f;

  if (npos > 0) {
    if (is_loader) {
      // ================================ loader wave ============================================
      // Streams load indices q = 0..npos in order.  Slot of q is q % nslots; it may be rewritten
      // once every consumer is past position q - nslots (positions < min progress are done).
      // Every slice is exactly `chunks` DMA wave-instructions, so the in-order vmcnt tells which
      // slices have landed.  The window image is flat on a fixed pitch, so the (row, column) a
      // lane serves -- its source offset inside the window -- is the same in every group of rows
      // and every slice, and a chunk costs the wave a few scalar instructions, two compares (the
      // slice's own extent masks the lanes it does not need) + one global_load_lds: measured with
      // tools/dma_probe.hip,
      // ONE such wave per CU streams 5.2-5.9 TB/s chip-wide (94-104 cycles per KiB), while a
      // compiler-scheduled loop with per-lane address arithmetic stays at ~415 cycles per KiB
      // whatever the memory behind it -- instruction issue, not HBM, is what a loader must save.
      __builtin_amdgcn_s_setprio(3);  // the stream must never wait for issue slots behind pollers
      const char *gv = reinterpret_cast<const char *>(Q.vox);
      // row groups g = lid, lid+NL, ... of every slice are mine; a group is `per` chunks = `rpg` rows
      const int per = Q.per, rpg = Q.rpg, groups = Q.groups;
      const int sg = lid % NLG;          // my slices: sg, sg + NLG, ...
      const int gl = lid / NLG, gn = LPG;  // my first row group of such a slice, and the stride to my next one
      const int mygroups = (groups - gl + gn - 1) / gn;
      const int mych = mygroups * per;  // DMA wave-instructions of a whole window (this loader's share)
      const unsigned strideVb = (unsigned)(Q.strideV * (long long)VB);  // bytes, < 2^32
      // unit 64*k + lane of a group sits at (row, column) = divmod(64*k + lane, wp): fixed per lane and phase k
      unsigned voff[7], rowk[7], colk[7];
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const unsigned g = 64u * k + lane;
        rowk[k] = g / (unsigned)Q.wp;
        colk[k] = g - rowk[k] * (unsigned)Q.wp;
        voff[k] = rowk[k] * strideVb + colk[k] * 16u;
      }
      const size_t gstep = (size_t)(gn * rpg) * strideVb;  // source advance from one of my groups to the next
      const size_t strideSb = (size_t)Q.strideS * VB;
      const bool l2hot = DIAG && (P.lockstep & 8) != 0;           // (diagnostic: every slice re-reads one slice)
      // (ALT: q runs over MY slices lid, lid + NL, ...; `landed` stays the published word: every slice below it that is
      //  mine has landed, so the minimum over the loaders' words is the complete prefix as before)
      int q = sg, inflight = 0, landed = sg, idle = 0, minp = 0, slot_q = sg % nslots, fly_total = 0;
      int fly_counts = 0;  // lane (q & 63): DMA wave-instructions of load index q (a scalar array in one VGPR)
      if (DIAG && (P.lockstep & 64)) minp = 0x3ffffff0;  // (diagnostic: free-running stream, nobody consumes)
      // progress words, read by lane 0 alone (NW <= 16 words as four b128 reads)
      auto poll_progress = [&]() -> int {
        int v = SLAB_DONE;
        if (lane < 16) v = raw_lds_b32(&ctl[8 + lane]);  // words >= NW stay at SLAB_DONE
        v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));
        v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));
        v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));
        v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));
        return __builtin_amdgcn_readlane(v, 0);
      };
      // one LDS-DMA wave-instruction: 16 B per active lane from src + voff to LDS dst + lane*16
      // (saddr form: no per-chunk VALU; M0 written in the statement that reads it)
      unsigned keep_m0;
#define SLAB_DMA(src_, dst_, voff_)                                                                                 \
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0" \
               : "=&s"(keep_m0)                                                                                     \
               : "v"(voff_), "s"(dst_), "s"(src_)                                                                   \
               : "memory")
      // table entries of 64 consecutive load indices, one per lane, refreshed every 64 slices:
      // a slice's window origin is then one v_readlane away instead of an LDS round trip
      // (Measured and dropped in round 2: the 64-bit source offset as two more lane arrays, and the
      //  column masks cached across slices in a VGPR bit set -- 1024^3 3.54 -> 3.74 ms: the scalar
      //  per-slice arithmetic below is cheaper than it looks, the extra VALU is not.)
      int ent_uv = 0, tab_base = -64;
      int ent_run = 0;  // ... and, for a slice nobody needs, the length of the run of empty layers it starts (EMPTY LAYERS)
      int n_skipped = 0;
      // EAGER PUBLICATION.  A slice used to be published when its loader, done issuing the NEXT one, waited
      // for it -- up to a slice's issue time (~0.5 us) after it had landed, on a ring that is a few slices
      // deep.  The wave's outstanding vector-memory count can be READ (s_getreg HW_REG_IB_STS: VM_CNT in
      // bits [3:0], its two high bits in [23:22]; tools/vmcnt_probe.hip), and the DMAs complete in order:
      // after every group of chunks the loader looks, and publishes each in-flight slice whose last
      // instruction is no longer outstanding.  `cur` = instructions of the slice being issued so far
      // (younger than everything in flight).  The blocking wait stays for when nothing can be issued.
      // (big workgroups only: on the small ones' deep ring a late word costs little, and the look costs
      //  the kernel scalar registers -- 97 spilled SGPRs against 39)
      constexpr bool EAGER = BIG;
      auto publish_landed = [&](int cur) {
        if (!EAGER || inflight == 0) return;
        const unsigned st = __builtin_amdgcn_s_getreg((31 << 11) | 7);
        const int out = (int)((st & 0xfu) | (((st >> 22) & 3u) << 4));
        const int before = landed;
        while (inflight > 0) {
          const int c_old = FIFO ? __builtin_amdgcn_readlane(fly_counts, (q - inflight * QSTEP) & 63) : mych;
          const int younger = (FIFO ? fly_total : mych * inflight) - c_old + cur;
          if (out > younger) break;
          if (FIFO) fly_total -= c_old;
          --inflight;
          landed += QSTEP;
        }
        if (landed != before) raw_lds_st_b32(&ctl[(lid < 4 ? 4 : 20) + lid], landed);
      };
      const bool prof = DIAG && (P.lockstep & 48) != 0 && Q.diag != nullptr;  // (diagnostic: where a loader's cycles go)
      long long t_issue = 0, t_wait = 0, t_idle = 0, t_mark = 0;
      const long long t_start = prof ? (long long)__builtin_amdgcn_s_memtime() : 0;
      while (landed <= npos) {
        // ---- issue while the ring has room (progress is re-polled only when it blocks us)
        bool stop = false;
        if (prof) t_mark = __builtin_amdgcn_s_memtime();
        while (q <= npos && inflight < Q.maxfly) {
          if ((q & ~63) != tab_base) {  // (q steps by QSTEP: entering a new block of 64 load indices, not hitting its first one)
            tab_base = q & ~63;
            const int ql = tab_base + lane;
            const int e = (dir > 0 ? smin + ql : smax + 1 - ql) - Q.Os;
            ent_uv = -1;
            ent_run = 0;
            if (ql <= npos && e >= 0 && e < Q.Ds) {
              const auto ent = raw_lds_b64(&wtab[e]);
              ent_uv = (int)ent.y;  // (.pack; never -1: u0 < 2^11)
              if (((int)ent.x & 3) == 3) ent_run = (int)ent.x >> 2;
            }
          }
          // EMPTY LAYERS.  A slice nobody samples is not streamed, and a whole run of them is stepped over at once: the
          // entry of an unneeded slice holds how many empty layers follow one another from its own on, and a slice between
          // two empty layers is unneeded.  Nothing is written, so no ring room is asked for.  Slices in flight are waited
          // for first when the run is long (their words are published in order); a short run behind slices in flight
          // goes slice by slice below.
          // (slice q + k lies between the layers of positions q + k - 1 and q + k when the march goes up the slice index,
          //  q + k and q + k + 1 when it goes down: there the last slice of the run borders the layer behind it)
          int run = flags ? __builtin_amdgcn_readlane(ent_run, q & 63) : 0;
          if (dir < 0 && run > 1) --run;
          run = min(run, npos + 1 - q);
          if (run > 0 && (inflight == 0 || run >= 8)) {
            if (inflight > 0) {
              wait_vmcnt(0);
              landed += inflight * QSTEP;
              inflight = 0;
              if (FIFO) fly_total = 0;
            }
            const int mine = (run + QSTEP - 1) / QSTEP;  // my slices among q .. q + run - 1
            if (gl == 0) n_skipped += mine;
            q += mine * QSTEP;
            landed = q;
            raw_lds_st_b32(&ctl[(lid < 4 ? 4 : 20) + lid], landed);
            slot_q = q % nslots;
            continue;
          }
          if (q - nslots >= minp) {
            minp = poll_progress();
            if (DIAG && (P.lockstep & 64)) minp = 0x3ffffff0;
            if (minp >= SLAB_DONE) {  // every consumer finished: the rest is not needed
              stop = true;
              break;
            }
            if (q - nslots >= minp) break;
          }
          const int uv = __builtin_amdgcn_readlane(ent_uv, q & 63);
          // Small windows count on every slice being the same number of DMA instructions (the in-order vmcnt): there an
          // unneeded slice may issue nothing only while none is in flight before it -- else it goes the uniform way with
          // `mych` one-unit reads.
          bool skip = run > 0;
          if (!FIFO && inflight > 0) skip = false;
          if (skip && gl == 0) ++n_skipped;
          int issued = 0;  // DMA wave-instructions of this slice (this loader's share)
          const unsigned dst0 = ring_addr + (unsigned)(slot_q * Q.slot_bytes + gl * per * 1024);
          if (skip) {
            // nothing
          } else if (uv != -1) {
            // (small windows: the whole shape -- the saving would not pay for the partial-group path)
            const unsigned need_u = Q.mask_need ? (((unsigned)uv >> 22) & 0x3fu) + 1u : (unsigned)Q.wu;
            const unsigned need_v = Q.mask_need ? (unsigned)Q.wv - ((unsigned)uv >> 28) * (unsigned)((Q.wv + 15) / 16) : (unsigned)Q.wv;
            const int sl = (dir > 0 ? smin + q : smax + 1 - q) - Q.Os;
            const unsigned u0 = (unsigned)uv & 0x7ffu, v0 = ((unsigned)uv >> 11) & 0x7ffu;
            const char *src = gv + (l2hot ? (size_t)0 : (size_t)sl * strideSb) + ((size_t)v0 * strideVb + (size_t)u0 * VB) +  // (64-bit: v0 * strideVb passes 4 GiB when V is the slowest axis of a 1024^3 volume)
                              (size_t)(gl * rpg) * strideVb;
            unsigned dst = dst0, row0 = (unsigned)(gl * rpg);
            // per = wp / gcd(64, wp) is 1, 3, 5 or 7 (the host picks such a pitch)
#define SLAB_GROUP(CHUNK)              \
  CHUNK(0)                             \
  if (per >= 3) {                      \
    CHUNK(1) CHUNK(2)                  \
    if (per >= 5) {                    \
      CHUNK(3) CHUNK(4)                \
      if (per >= 7) { CHUNK(5) CHUNK(6) } \
    }                                  \
  }
            // Lanes outside what THIS slice needs of the window stay idle (the fixed shape is sized
            // for the widest section of the bundle; at a voxel per pixel the mean need is ~70 % of
            // it).  Column masks are per slice; groups past the needed rows are not issued at all;
            // only the group the needed rows end in pays a per-lane row test (lane 0 always loads
            // there, so that a group is `per` wave-instructions: the in-order vmcnt counts slices
            // through the per-slice instruction counts kept in fly_counts).
            bool cm[7];
            unsigned long long mk[7];  // the same column masks as wave-uniform lane masks (EXEC values)
#pragma unroll
            for (int k = 0; k < 7; ++k) {
              cm[k] = k < per && colk[k] < need_u;
              mk[k] = __builtin_amdgcn_ballot_w64(cm[k]);
            }
#define CM(k) cm[k]
            for (int g = 0; g < mygroups; ++g) {
              if (FIFO && row0 >= need_v) break;  // nothing of this group (or the following ones) is needed: not issued, not counted
              issued += per;
              // (small workgroups issue every row group of the window whatever the slice needs of it -- the instruction
              //  count is the same either way -- so a group that lies inside the window goes the branch-free way even
              //  when its last rows are not needed; the host makes the window a whole number of groups where it can)
              if (row0 + (unsigned)rpg <= (BIG ? need_v : (unsigned)Q.wv)) {
                if (per == 3) {
                  // a whole group in ONE statement: EXEC takes each chunk's column mask in turn, M0 steps
                  // through the chunks' LDS images -- three scalar instructions per chunk and no branch
                  // (every chunk has a column-0 lane, so no mask is empty)
                  unsigned long long keep_exec;
                  asm volatile("s_mov_b32 %[km], m0\n\ts_mov_b64 %[ke], exec\n\ts_mov_b32 m0, %[dst]\n\t"
                               "s_mov_b64 exec, %[e0]\n\tglobal_load_lds_dwordx4 %[v0], %[src]\n\ts_add_u32 m0, m0, 0x400\n\t"
                               "s_mov_b64 exec, %[e1]\n\tglobal_load_lds_dwordx4 %[v1], %[src]\n\ts_add_u32 m0, m0, 0x400\n\t"
                               "s_mov_b64 exec, %[e2]\n\tglobal_load_lds_dwordx4 %[v2], %[src]\n\t"
                               "s_mov_b64 exec, %[ke]\n\ts_mov_b32 m0, %[km]"
                               : [km] "=&s"(keep_m0), [ke] "=&s"(keep_exec)
                               : [dst] "s"(dst), [src] "s"(src), [e0] "s"(mk[0]), [e1] "s"(mk[1]), [e2] "s"(mk[2]), [v0] "v"(voff[0]),
                                 [v1] "v"(voff[1]), [v2] "v"(voff[2])
                               : "memory", "scc");
                } else if (per == 1) {  // one chunk per group (pitches 8, 16, 32, 64): the same, once
                  unsigned long long keep_exec;
                  asm volatile("s_mov_b32 %[km], m0\n\ts_mov_b64 %[ke], exec\n\ts_mov_b32 m0, %[dst]\n\t"
                               "s_mov_b64 exec, %[e0]\n\tglobal_load_lds_dwordx4 %[v0], %[src]\n\t"
                               "s_mov_b64 exec, %[ke]\n\ts_mov_b32 m0, %[km]"
                               : [km] "=&s"(keep_m0), [ke] "=&s"(keep_exec)
                               : [dst] "s"(dst), [src] "s"(src), [e0] "s"(mk[0]), [v0] "v"(voff[0])
                               : "memory", "scc");
                } else {
#define SLAB_CHUNK_ROWS_OK(k) \
  if (CM(k)) SLAB_DMA(src, dst + k * 1024u, voff[k]);
                  SLAB_GROUP(SLAB_CHUNK_ROWS_OK)
#undef SLAB_CHUNK_ROWS_OK
                }
              } else {
#define SLAB_CHUNK_MASKED(k)                                                                  \
  {                                                                                           \
    const bool in_need = CM(k) && row0 + rowk[k] < need_v;                                    \
    const unsigned vo = in_need ? voff[k] : 0u; /* lane 0 re-reads the group's first unit */  \
    if (in_need || lane == 0) SLAB_DMA(src, dst + k * 1024u, vo);                             \
  }
                SLAB_GROUP(SLAB_CHUNK_MASKED)
#undef SLAB_CHUNK_MASKED
              }
              src += gstep;
              dst += (unsigned)(gn * per * 1024);
              row0 += (unsigned)(gn * rpg);
              publish_landed(issued);
            }
#undef SLAB_GROUP
#undef CM
          } else if (!FIFO) {
            // slice outside the stored box (never read): uniform counting wants its instructions all the same
            unsigned dst = dst0;
            for (int c = 0; c < mych; ++c) {
              SLAB_DMA(gv, dst, voff[0] * 0u);
              dst += 1024u;
            }
          }
          if (FIFO) {  // big windows: slices differ in what they issue, the counts are kept per slice
            fly_counts = lane == (q & 63) ? issued : fly_counts;
            fly_total += issued;
          }
          q += QSTEP;
          ++inflight;
          slot_q += QSTEP;
          if (slot_q >= nslots) slot_q -= nslots;  // (QSTEP <= 8 < 3 <= nslots is not guaranteed: see the host's ring check)
        }
        if (prof) {
          const long long t = __builtin_amdgcn_s_memtime();
          t_issue += t - t_mark;
          t_mark = t;
        }
        if (stop) break;
        publish_landed(0);
        if (EAGER && inflight < Q.maxfly && q <= npos && q - nslots < minp) continue;  // room again: issue on
        if (inflight > 0) {
          // retire the oldest slice in flight: everything but the younger slices' DMAs is done
          if (FIFO) {
            fly_total -= __builtin_amdgcn_readlane(fly_counts, (q - inflight * QSTEP) & 63);
            wait_vmcnt(fly_total);
          } else {
            wait_vmcnt(mych * (inflight - 1));  // small windows: every slice is mych wave-instructions
          }
          --inflight;
          landed += QSTEP;
          raw_lds_st_b32(&ctl[(lid < 4 ? 4 : 20) + lid], landed);
          if (prof) t_wait += (long long)__builtin_amdgcn_s_memtime() - t_mark;
        } else {
          const int flagged = raw_lds_b32(&ctl[3]);
          if (++idle > (1 << 22) || flagged) {  // bounded spin (see consumers)
            if (!flagged) raw_lds_st_b32(&ctl[3], 1);  // (a violated window bound stays the reported cause)
            break;
          }
          __builtin_amdgcn_s_sleep(1);
          if (prof) t_idle += (long long)__builtin_amdgcn_s_memtime() - t_mark;
        }
      }
#undef SLAB_DMA
      wait_vmcnt(0);
      if (n_skipped && lane == 0) atomicAdd(&ctl[2], n_skipped);
      if (tracing && !phases && lane == 0 && lid == 0) {
        unsigned *t = Q.trace + 8 * (size_t)blockIdx.x;
        t[4] = (unsigned)(t_issue >> 6);
        t[5] = (unsigned)(t_wait >> 6);
        t[6] = (unsigned)(t_idle >> 6);
      }
      if (prof && lane == 0 && lid == 0) {
        atomicAdd(&Q.diag[4], (float)t_issue * 1e-3f);
        atomicAdd(&Q.diag[5], (float)t_wait * 1e-3f);
        atomicAdd(&Q.diag[6], (float)t_idle * 1e-3f);
        atomicAdd(&Q.diag[7], (float)((long long)__builtin_amdgcn_s_memtime() - t_start) * 1e-3f);
      }
    } else {
      // ================================ consumer waves ==========================================
      // One sample per lane and iteration.  A lane takes its next sample as soon as the two
      // slices it touches have landed; the wave's progress is the position of its slowest lane.
      // While data is ahead of the wave every unfinished lane is active in every iteration (a
      // fixed slice step per iteration would leave the lanes without a sample in it idle).
      // slices landed = the slowest loader's count
      // (one 16-byte LDS read per poll: the four words are adjacent and aligned)
      auto landed_all = [&]() -> int {
        int4 v;
        const unsigned a = (unsigned)(size_t)(lds_cptr_t)(ctl + 4);
        if constexpr (NL > 4) {  // loaders 4..7 publish at ctl[24..27] (words that stay at SLAB_DONE when unused)
          int4 w;
          asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:80\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v), "=&v"(w) : "v"(a) : "memory");
          return min(min(min(v.x, v.y), min(v.z, v.w)), min(min(w.x, w.y), min(w.z, w.w)));
        }
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
        return min(min(v.x, v.y), min(v.z, v.w));
      };
      const bool stream_only = DIAG && (P.lockstep & 2) != 0;  // (diagnostic: consume nothing)
      if (DIAG && (P.lockstep & 64)) pb = SLAB_DONE;   // (diagnostic: free-running stream)
      const bool count = DIAG && (P.lockstep & 48) != 0 && Q.diag != nullptr;
      float n_it = 0.f, n_act = 0.f, n_in = 0.f, n_hit = 0.f, n_anyhit = 0.f, n_lead = 0.f, n_waits = 0.f, n_wstep = 0.f;
      float n_work = 0.f, n_own = 0.f;
      // (turns in which some lane's occupancy bit is set -- the visible path runs --, the cycles of that path, from the issue
      //  of the table loads to the blend, and the cycles of them spent waiting for the texels: two time stamps each)
      float n_anymaybe = 0.f, c_vis = 0.f, c_texwait = 0.f;
      // (diagnostic: wait for the texels where they are issued, as the kernel did before the normal work moved under them)
      const bool texwait_at_issue = count && (P.lockstep & 512) != 0;
      int have = 0;  // cached copy of `landed` (monotonic): re-polled only when a lane is blocked on it
      const float inv_bs = 1.0f / B[AS];  // (planes per slice along this ray; the principal axis' B is never 0)
      // table row of the sample's base slice: entry index = bs - Os = psgn*pb + (-psgn*poff - Os)
      const int eoff = -psgn * poff - Q.Os;
      const unsigned wtab_addr = (unsigned)(size_t)(lds_cptr_t)wtab;
      // (LEAN: as a byte offset from the ring's start with entry 0's folded in -- one multiply-add per turn finds the entry)
      const int tab0 = (int)(wtab_addr - ring_addr) + 8 * eoff, psgn8 = 8 * psgn;
      for (int it = 0;; ++it) {
        SLAB_MARK("loop head");
        const bool want = pb < SLAB_DONE;
        if (!__any(want)) break;  // every ray of this wave is finished
        // progress = position of the slowest lane (DPP reduction, 8 VALU in the plain frames' instances), published every
        // iteration on a short ring and every other one where a stale value only delays slot
        // recycling by a step
        if (!EARLY && !(it & Q.pmask)) {
          const int plo = wave_min_i32<TURN>(pb);
          if (plo != pos) {  // positions below plo are done: their lower slices may be recycled
            pos = plo;       // (every slot read of earlier iterations has returned: slab_read8 waits)
            if (lane == 0) lds_st(&ctl[8 + wave], pos);
          }
        }
        // Take a step only when the whole band of this wave can: lanes sit up to one sample
        // spacing (wstep slices) ahead of the slowest one, and an iteration costs the wave the
        // same issue slots whether 5 or 64 lanes take part.  Stepping the moment ONE lane's slices
        // have landed was measured at up to 2.3x the iterations per ray on a starved stream.
        int need = min(pos + 2 + Q.wstep, npos + 1);
        if (have < need) {
          have = landed_all();
          if (have < need) {
            // make sure `pos` is this wave's true minimum before sleeping on it
            const int plo = wave_min_i32<TURN>(pb);
            if (plo != pos) {
              pos = plo;
              if (lane == 0) lds_st(&ctl[8 + wave], pos);
              need = min(pos + 2 + Q.wstep, npos + 1);
            }
            if (count) n_waits += 1.f;
            for (int spins = 0; have < need; ++spins) {
              const int flagged = lds_ld(&ctl[3]);
              if (spins > (1 << 22) || flagged) {  // bounded: never hang the GPU on a protocol bug
                if (!flagged) lds_st(&ctl[3], 1);
                have = 0x3ffffff0;
                m1 = m - 1;
                pb = SLAB_DONE;
                break;
              }
              // (backing off further for waves whose first slice is many slices away was measured
              //  slower: reaction time matters more than the polls' issue slots)
              __builtin_amdgcn_s_sleep(SLAB_POLL_SLEEP);
              have = landed_all();
            }
          }
          have = __builtin_amdgcn_readfirstlane(have);
        }
        // (Measured and dropped: several samples per lane and turn of the loop, to pay the loop's own
        //  cost -- progress word, poll, flow control -- once per two or three samples.  512^3 f32 frame,
        //  1 / 2 / 3 samples: 1.89 / 2.02 / 1.97 ms; the scalar instruction count did not move (4.74e8 ->
        //  4.81e8) and the vector one rose 12 %: lanes whose next slices have not landed sit the extra
        //  sample out, so the second body mostly runs with few lanes.)
        // (one sample per turn; the body stays a one-turn loop: as a plain block it changes the register allocation of
        //  the u8 colour-table instances)
#pragma unroll
        for (int rep = 0; rep < 1; ++rep) {
        const bool act = pb < SLAB_DONE && pb + 2 <= have;
        if (count) {
          n_lead += (float)(have - pos);
          n_wstep += (float)Q.wstep;
        }
        asm volatile("" ::: "memory");  // slot reads stay behind the poll
        bool d_hit = false, d_own = false, d_maybe = false;  // (diagnostic counters only)
        unsigned d_t0 = 0, d_vis = 0, d_wait = 0;
        // ---- part A: where the sample is and its corner addresses; EARLY: the whole corner batch
        float fx = 0.f, fy = 0.f, fz = 0.f;
        unsigned a0 = 0, b0 = 0;
        typename std::conditional<DT != 1, v2u, v4f>::type rq[EARLY ? 8 : 1];
        float early_nsc = 0.f;
        int early_ni = 0;
        bool work = act && !stream_only;
        int base_a = 0, base_b = 0;
        if (work) {
          // the two slices' slot images (one 8-byte table entry each, adjacent): issued first,
          // the position arithmetic below covers the LDS round trip
          const int *te = LEAN ? reinterpret_cast<const int *>(smem + (unsigned)(__mul24(psgn8, pb) + tab0))
                               : reinterpret_cast<const int *>(smem + (wtab_addr - ring_addr)) + 2 * (__mul24(psgn, pb) + eoff);  // (24-bit multiply: full rate; |pb| < 4096 on a lane that works)
          base_a = te[0];
          base_b = BR ? (te[2] & ~1) : te[2];  // (bit 0: the NEXT layer's flag)
        }
        // EMPTY LAYERS: nothing in this sample's layer can be visible for any ray of the tile -- the sample is exactly
        // transparent, and its slices may not even have been streamed
        // (TURN: no test of `flags` here or below.  Without brick flags nobody sets the entries' low bits, and the base
        //  addresses are multiples of 8 -- smem is 16-byte aligned, a slot is whole KiB, a row 16 bytes, a voxel VB: the bits read 0.  As a run-time switch it was two lane masks held in scalar registers
        //  through the loop and three v_cndmask 0, 1 per turn to apply them to `work`)
        if constexpr (TURN) {
          if constexpr (BR) work = work && !(base_a & 1);
        } else if (flags) work = work && !(base_a & 1);
        // the plane of this ray's next sample: the next one, or -- from a layer that starts a run of empty ones (the
        // entry holds its length, see the set-up) -- the first plane whose base slice lies behind the run.  The planes
        // in between fall into empty layers, all of them: positions are monotone in the plane index.
        int m_next = m + 1;
        if ((TURN ? BR : flags) && act && (base_a & 3) == 3) {
          const int ptar = pb + (base_a >> 2);  // first position behind the run
          if (ptar >= npos) m_next = m1 + 1;    // nothing but empty layers to the end of the tile's range
          else {
            // s(m) = fma(m, B, A) reaches the target slice at m = t; floor(t) is never behind the exact answer (the
            // division is off by far less than a plane), the exact base slices of the planes from there on decide
            const float starget = (float)(dir > 0 ? smin + ptar : smax - ptar + 1);
            int mj = max((int)floorf((starget - A[AS]) * inv_bs), m + 1);
#pragma unroll 1
            for (int k = 0; k < 4 && mj <= m1; ++k) {
              if (__mul24(psgn, base_slice(mj)) + poff >= ptar) break;
              ++mj;
            }
            m_next = mj;
          }
        }
        if (work) {
          const float mf = (float)m;
          // (no membership test: [m, m1] is exactly the inside interval, see the set-up)
          // (the principal axis' clamped coordinate and base index were computed when this sample's position in
          //  the stream was: fma(m, B, A) -> clamp -> min((int), N - 2), the very operations of smk_lin_clamp)
          int x0 = 0, x1, y0 = 0, y1, z0 = 0, z1;
          if constexpr (AS != 0) smk_lin_clamp(__fmaf_rn(mf, B[0], A[0]), P.N[0], x0, x1, fx);
          else { x0 = car_i; fx = car_sc - (float)car_i; }
          if constexpr (AS != 1) smk_lin_clamp(__fmaf_rn(mf, B[1], A[1]), P.N[1], y0, y1, fy);
          else { y0 = car_i; fy = car_sc - (float)car_i; }
          if constexpr (AS != 2) smk_lin_clamp(__fmaf_rn(mf, B[2], A[2]), P.N[2], z0, z1, fz);
          else { z0 = car_i; fz = car_sc - (float)car_i; }
          (void)x1; (void)y1; (void)z1;
          const int iu = AU == 0 ? x0 : y0, iv = AV == 1 ? y0 : z0;  // global voxel indices
          if (count && flags)  // (diagnostic: would this lane's OWN brick have let it skip the sample?)
            d_own = Q.bricks[(size_t)((car_i - Q.Os) >> SMK_BRICK_LOG2) * Q.bss + (size_t)((iv - Q.Ov) >> SMK_BRICK_LOG2) * Q.bsv +
                             (size_t)((iu - Q.Ou) >> SMK_BRICK_LOG2) * Q.bsu] != 0;
          const unsigned lo_off = __umul24((unsigned)iv, pitch_b) + ((unsigned)iu << VBL);  // (24-bit multiply: full rate)
          a0 = (unsigned)base_a + lo_off;
          b0 = (unsigned)base_b + lo_off;
          if constexpr (EARLY) slab_read8_full(a0, a0 + pitch_b, b0, b0 + pitch_b, rq);
        }
        if constexpr (EARLY) {
          // everything this iteration needs of the ring is in registers: release the slots NOW, not
          // a classification + shading later -- on a 5-slot ring the loaders otherwise sit blocked
          // for most of the consumers' iteration
          int pbn = pb;
          float nsc = car_sc;
          int ni = car_i;
          if (act) {
            if (m_next <= m1) {
              ni = base_slice_c(m_next, nsc);
              pbn = __mul24(psgn, ni) + poff;
            } else pbn = SLAB_DONE;
          }
          early_nsc = nsc;
          early_ni = ni;
          // (every turn: on the 5-slot ring a progress word that is one turn late costs 16 % -- 4.07 vs 4.71 ms)
          const int plo = wave_min_i32<TURN>(pbn);
          if (plo != pos && plo < SLAB_DONE) {
            pos = plo;
            if (lane == 0) lds_st(&ctl[8 + wave], pos);
          }
        }
        if (work) {
          // corners <ds><dv><du> -> model order <dx><dy><dz>; lerp order x, y, z like the gather kernel
#define QI(dx, dy, dz) (PERM == 0 ? ((dz) * 4 + (dy) * 2 + (dx)) : PERM == 1 ? ((dy) * 4 + (dz) * 2 + (dx)) : ((dx) * 4 + (dz) * 2 + (dy)))
#define TRI(E)                                                                                                             \
  smk_lerp(smk_lerp(smk_lerp(E(0, 0, 0), E(1, 0, 0), fx), smk_lerp(E(0, 1, 0), E(1, 1, 0), fx), fy),                       \
           smk_lerp(smk_lerp(E(0, 0, 1), E(1, 0, 1), fx), smk_lerp(E(0, 1, 1), E(1, 1, 1), fx), fy), fz)
          float ch0, ch1, ch2 = 0.f, ch3 = 0.f;
          // big workgroups, float voxels, separable table: the third channel is only looked at behind the (v, g) quad's
          // occupancy bit -- one sample in fourteen on the 1024^3 frame -- and its corners are in registers anyway, so
          // its interpolation (14 packed instructions) waits until then
          // (small workgroups: the ring slots are still held, so the third channel is READ only then, too: 8 x 8 bytes
          //  per sample instead of 8 x 12)
          // (byte voxels: all four channels come in one word per corner, the interpolation alone is deferred)
          const bool lazy_h = (TF == 1 && Q.fast_tf) || (TF == 2 && Q.use_occ);
          uint32_t q8[DT != 1 && !EARLY ? 8 : 1];  // small workgroups, 8-byte voxels: the corners' data words
          auto tri_h_early = [&]() -> float {
            if constexpr (EARLY && DT == 2) {  // u16 voxels: the third channel's 8 bits ride above the normal (smk_decode_u16)
#define E2(dx, dy, dz) (float)(rq[QI(dx, dy, dz)].y >> 24)
              return TRI(E2) * SMK_INV255;
#undef E2
            } else if constexpr (DT == 2) {
              uint32_t hq[8];
              slab_read8_nb8<LEAN>(a0, a0 + pitch_b, b0, b0 + pitch_b, hq);
#define E2(dx, dy, dz) (float)(hq[QI(dx, dy, dz)] >> 24)
              return TRI(E2) * SMK_INV255;
#undef E2
            } else if constexpr (EARLY && DT == 0) {
#define E2(dx, dy, dz) smk_ub(rq[QI(dx, dy, dz)].x, 2)
              return TRI(E2) * SMK_INV255;
#undef E2
            } else if constexpr (DT == 0) {
#define E2(dx, dy, dz) smk_ub(q8[QI(dx, dy, dz)], 2)
              return TRI(E2) * SMK_INV255;
#undef E2
            } else if constexpr (EARLY && DT == 1) {
#define E2(dx, dy, dz) rq[QI(dx, dy, dz)].z
              return TRI(E2);
#undef E2
            } else if constexpr (DT == 1) {
              uint32_t hq[8];
              slab_read8_h16<LEAN>(a0, a0 + pitch_b, b0, b0 + pitch_b, hq);
#define E2(dx, dy, dz) __uint_as_float(hq[QI(dx, dy, dz)])
              return TRI(E2);
#undef E2
            } else {
              return 0.f;
            }
          };
          if constexpr (DT == 2) {
            // u16 voxels: both 16-bit channels in the data word, interpolated raw and scaled once (the gather kernel's
            // operations); the third channel as tri_h_early reads it
            if constexpr (!EARLY) slab_read8_u8(a0, a0 + pitch_b, b0, b0 + pitch_b, q8);
#define W16(dx, dy, dz) (EARLY ? rq[EARLY ? QI(dx, dy, dz) : 0].x : q8[EARLY ? 0 : QI(dx, dy, dz)])
#define E0(dx, dy, dz) (float)(W16(dx, dy, dz) & 0xffffu)
#define E1(dx, dy, dz) (float)(W16(dx, dy, dz) >> 16)
            ch0 = TRI(E0) * SMK_INV65535;
            ch1 = TRI(E1) * SMK_INV65535;
            if ((TF == 2 || P.third_axis) && !lazy_h) ch2 = tri_h_early();
#undef E1
#undef E0
#undef W16
          } else if constexpr (EARLY && DT == 1) {
#define E0(dx, dy, dz) rq[QI(dx, dy, dz)].x
#define E1(dx, dy, dz) rq[QI(dx, dy, dz)].y
            ch0 = TRI(E0);
            ch1 = TRI(E1);
            if ((TF == 2 || P.third_axis) && !lazy_h) ch2 = tri_h_early();
#undef E1
#undef E0
          } else if constexpr (EARLY && DT == 0) {
#define E0(dx, dy, dz) smk_ub(rq[QI(dx, dy, dz)].x, 0)
#define E1(dx, dy, dz) smk_ub(rq[QI(dx, dy, dz)].x, 1)
#define E2(dx, dy, dz) smk_ub(rq[QI(dx, dy, dz)].x, 2)
#define E3(dx, dy, dz) smk_ub(rq[QI(dx, dy, dz)].x, 3)
            ch0 = TRI(E0) * SMK_INV255;
            ch1 = TRI(E1) * SMK_INV255;
            if ((TF == 2 || P.third_axis) && !lazy_h) {
              ch2 = TRI(E2) * SMK_INV255;
              if (P.nelts == 4) ch3 = TRI(E3) * SMK_INV255;
            }
#undef E3
#undef E2
#undef E1
#undef E0
          } else if constexpr (DT == 1) {
            if ((TF == 2 || P.third_axis) && !lazy_h) {
              v3f q[8];
              slab_read8(a0, a0 + pitch_b, b0, b0 + pitch_b, q);
#define E0(dx, dy, dz) q[QI(dx, dy, dz)].x
#define E1(dx, dy, dz) q[QI(dx, dy, dz)].y
#define E2(dx, dy, dz) q[QI(dx, dy, dz)].z
              ch0 = TRI(E0);
              ch1 = TRI(E1);
              ch2 = TRI(E2);
#undef E2
            } else {
              v2f q[8];
              slab_read8(a0, a0 + pitch_b, b0, b0 + pitch_b, q);
              ch0 = TRI(E0);
              ch1 = TRI(E1);
#undef E1
#undef E0
            }
          } else {
            uint32_t (&q)[DT != 1 && !EARLY ? 8 : 1] = q8;
            if constexpr (DT == 0 && !EARLY) slab_read8_u8(a0, a0 + pitch_b, b0, b0 + pitch_b, q8);
#define E0(dx, dy, dz) smk_ub(q[QI(dx, dy, dz)], 0)
#define E1(dx, dy, dz) smk_ub(q[QI(dx, dy, dz)], 1)
#define E2(dx, dy, dz) smk_ub(q[QI(dx, dy, dz)], 2)
#define E3(dx, dy, dz) smk_ub(q[QI(dx, dy, dz)], 3)
            ch0 = TRI(E0) * SMK_INV255;
            ch1 = TRI(E1) * SMK_INV255;
            if ((TF == 2 || P.third_axis) && !lazy_h) {
              ch2 = TRI(E2) * SMK_INV255;
              if (P.nelts == 4) ch3 = TRI(E3) * SMK_INV255;
            }
#undef E3
#undef E2
#undef E1
#undef E0
          }
#undef TRI
          // what the interpolated normal contributes to the Phong term (smk_shade_geom): the packed normals of the same
          // corners -- a second batch of LDS reads, or already here (EARLY) --, their interpolation, the two dot products
          auto phong_geom = [&]() -> SmkPhong {
            uint32_t nb[8];
            if constexpr (EARLY) {
#pragma unroll
              for (int k = 0; k < 8; ++k) {
                if constexpr (DT == 1) nb[k] = __float_as_uint(rq[k].w);
                else nb[k] = rq[k].y;
              }
            } else if (DT == 1) slab_read8_nb16<LEAN>(a0, a0 + pitch_b, b0, b0 + pitch_b, nb);
            else slab_read8_nb8<LEAN>(a0, a0 + pitch_b, b0, b0 + pitch_b, nb);
#define NB(dx, dy, dz) nb[QI(dx, dy, dz)]
            float n0 = smk_nrm(NB(0, 0, 0), NB(1, 0, 0), NB(0, 1, 0), NB(1, 1, 0), NB(0, 0, 1), NB(1, 0, 1), NB(0, 1, 1), NB(1, 1, 1), 0, fx, fy, fz);
            float n1 = smk_nrm(NB(0, 0, 0), NB(1, 0, 0), NB(0, 1, 0), NB(1, 1, 0), NB(0, 0, 1), NB(1, 0, 1), NB(0, 1, 1), NB(1, 1, 1), 1, fx, fy, fz);
            float n2 = smk_nrm(NB(0, 0, 0), NB(1, 0, 0), NB(0, 1, 0), NB(1, 1, 0), NB(0, 0, 1), NB(1, 0, 1), NB(0, 1, 1), NB(1, 1, 1), 2, fx, fy, fz);
#undef NB
            return smk_shade_geom<SH>(P, n0, n1, n2);
          };
          // ---- classification and, for a sample that shows, everything behind it.  Two pieces of text that both arrangements
          // below share, as macros: the same tokens give the instances that keep the older arrangement the code they had.
          // (1) SLAB_FAST_ALPHA, the separable table's alpha from the issue of the texel loads on.
          //     SHADE UNDER THE FETCH.  The four texels come from L2; nothing of the normal's share of the Phong term needs
          //     them -- the second batch of LDS reads, 21 lerps, the rotation, rsqrt, two dot products and the specular power,
          //     the larger half of a visible sample's arithmetic -- so it runs behind the issue of the loads and in front of
          //     their first use.  (The asm statement of the LDS batch keeps the loads above it; the wait for them is the
          //     compiler's, in front of the alpha.)  A sample that then turns out to have alpha 0 paid it for nothing.
          //     Alpha first (all four (V,G) texels are needed for it anyway), times the third-axis alpha where that is in
          //     use (the same products as smk_classify); colour only on a hit.
#define SLAB_FAST_ALPHA \
  if (count) { \
    d_maybe = true; \
    d_t0 = (unsigned)__builtin_amdgcn_s_memtime(); \
  } \
  tx4 = slab_tex2d_fetch<LEAN>(P.tf_vg, P.sv, s0, t0, fs, ft); \
  if (texwait_at_issue) { \
    const unsigned t = (unsigned)__builtin_amdgcn_s_memtime(); \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    d_wait = (unsigned)__builtin_amdgcn_s_memtime() - t; \
  } \
  if constexpr (SH != 0) ph = phong_geom(); \
  if (count) { \
    const unsigned t = (unsigned)__builtin_amdgcn_s_memtime(); \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
    d_wait += (unsigned)__builtin_amdgcn_s_memtime() - t; \
  } \
  col.w = slab_tex_chan(tx4, 3); \
  if (Q.use_ah) { \
    if (lazy_h) ch2 = tri_h_early(); \
    int h0, h1; \
    float fh; \
    smk_lin_clamp(__fmaf_rn(ch2, (float)P.sv, -0.5f), P.sv, h0, h1, fh); \
    col.w *= smk_lerp(ah[h0], ah[h0 + 1], fh) * SMK_INV255; \
  } \
  col.w = smk_sat(col.w);
          // (2) SLAB_SHOW, a sample whose alpha is not 0: its colour; in frames with shadows the light-buffer colour over it, as
          //     the slices nearer the light left it (smk_shadow.hip; the sample's own position: the gather kernel's fma chain);
          //     shading (the 1-D colour table's entries are premultiplied, TLUT.cpp:65-71, as in the gather kernel; the
          //     separable table's path has the normal's share already); first-hit depth (the gather kernel's `first`): the
          //     first sample that passes classification finds the accumulated alpha still exactly 0, no later one does --
          //     nothing is carried through the loop for it; the blend.  GL_MAX (gluvvShadeMIP) has no order and no
          //     termination; otherwise exact early termination: once A == 1.0f every later weight (1-A) is exactly 0, so no
          //     later sample can change C or A.
#define SLAB_SHOW \
  if (TF == 1 && Q.fast_tf) { \
    col.x = slab_tex_chan(tx4, 0); \
    col.y = slab_tex_chan(tx4, 1); \
    col.z = slab_tex_chan(tx4, 2); \
  } \
  float4 src; \
  float shadow[3], keepf = 1.0f; \
  const float *shp = nullptr; \
  if (TF != 0 && SHD) { \
    const float mf = (float)m; \
    if constexpr (NVL) { \
      keepf = smk_shadow_keep(P, m, __fmaf_rn(mf, B[0], A[0]), __fmaf_rn(mf, B[1], A[1]), __fmaf_rn(mf, B[2], A[2])); \
    } else { \
      smk_shadow_term(P, m, __fmaf_rn(mf, B[0], A[0]), __fmaf_rn(mf, B[1], A[1]), __fmaf_rn(mf, B[2], A[2]), shadow); \
      shp = shadow; \
    } \
  } \
  if (TF == 0) { \
    src = col; \
  } else if (SH == 0) { \
    src = smk_shade_sample<0, NVL>(P, col, 0.f, 0.f, 0.f, 0.f, shp, keepf); \
  } else { \
    if (!(TF == 1 && Q.fast_tf)) ph = phong_geom(); \
    src = smk_shade_apply<SH, NVL>(P, col, ch1, ph, shp, keepf); \
  } \
  if (P.depth != nullptr && C3 == 0.0f) P.depth[(size_t)j * P.W + i] = smk_plane_depth_px<SHD>(P, m, px, py); \
  if (P.blend == SMK_BLEND_MAX) { \
    C0 = fmaxf(C0, src.x); \
    C1 = fmaxf(C1, src.y); \
    C2 = fmaxf(C2, src.z); \
    C3 = fmaxf(C3, src.w); \
  } else { \
    float w = 1.0f - C3; \
    C0 = __fmaf_rn(w, src.x, C0); \
    C1 = __fmaf_rn(w, src.y, C1); \
    C2 = __fmaf_rn(w, src.z, C2); \
    C3 = __fmaf_rn(w, src.w, C3); \
    if (C3 == 1.0f) m1 = m; \
  }
          if constexpr (TURN) {
            // ONE block behind the occupancy bit.  The bit of the sample's texel quad decides whether anything of a visible
            // sample runs at all: clear => alpha is exactly 0, and most samples of a typical transfer function end there,
            // without the L2 round trip.  Fetch, normal, alpha, colour, shading, first-hit depth and blend are nested inside
            // that one test, and what they hand on to each other (the texels, the Phong term, the colour) is declared inside
            // it.  Declared in front of it and used in a second block behind it -- the other arrangement -- every one of them
            // costs every turn of the loop a `v_mov 0` for the lanes that skip both blocks: nine in the separable table's turn
            // (*Instruction stream of a turn*).  The same operations in the same order.
            const bool fast = TF == 1 && Q.fast_tf;  // separable table: bilinear (V,G) lookup x optional third-axis alpha
            const bool occ3 = TF == 2 && Q.use_occ;  // dense 3-D table, its (v, g) bitmap folded over the sheets (smk_set_tf3d)
            int s0 = 0, s1, t0 = 0, t1;
            float fs = 0.f, ft = 0.f;
            bool maybe = true;  // (no bitmap: every sample goes on)
            if (fast) {
              smk_lin_clamp(__fmaf_rn(ch0, (float)P.sv, -0.5f), P.sv, s0, s1, fs);
              smk_lin_clamp(__fmaf_rn(ch1, (float)P.sg, -0.5f), P.sg, t0, t1, ft);
              if (Q.use_occ) maybe = (occ[__mul24(t0, P.occ_roww) + (s0 >> 5)] >> (s0 & 31)) & 1u;
            } else if (occ3) {
              smk_lin_clamp(__fmaf_rn(ch0, (float)P.s3v, -0.5f), P.s3v, s0, s1, fs);
              smk_lin_clamp(__fmaf_rn(ch1, (float)P.s3g, -0.5f), P.s3g, t0, t1, ft);
              maybe = (occ[__mul24(t0, P.occ_roww) + (s0 >> 5)] >> (s0 & 31)) & 1u;
            }
            (void)s1; (void)t1;
            if (maybe) {
              SLAB_MARK("occupancy bit");
              SmkPhong ph = {0.f, 0.f};
              float4 col;
              bool hit;
              SlabTexel4 tx4 = {0, 0, 0, 0, 0.f, 0.f};
              if (!fast) {
                if (occ3) ch2 = tri_h_early();  // (the third coordinate of the lookup: only behind the bit)
                hit = smk_classify<DT, TF>(P, ch0, ch1, ch2, ch3, col);
              } else {
                SLAB_FAST_ALPHA
                hit = col.w != 0.0f;
              }
              d_hit = hit;
              if (hit) {
                SLAB_SHOW
              }
            }
          } else {
            // (frames with shadows, scene depth or the NV20 look, and the diagnostic instances: two blocks, the carriers declared in front of both -- nested,
            //  instances that sit at the 80 VGPRs of their launch bound pass it: profiles/r06_turn_diet.md)
            SmkPhong ph = {0.f, 0.f};
            float4 col;
            bool hit;
            SlabTexel4 tx4 = {0, 0, 0, 0, 0.f, 0.f};
            if (TF == 1 && Q.fast_tf) {
              int s0, s1, t0, t1;
              float fs, ft;
              smk_lin_clamp(__fmaf_rn(ch0, (float)P.sv, -0.5f), P.sv, s0, s1, fs);
              smk_lin_clamp(__fmaf_rn(ch1, (float)P.sg, -0.5f), P.sg, t0, t1, ft);
              // occupancy bit of the texel quad (LDS): clear => alpha is exactly 0, no fetch.  Most
              // samples of a typical transfer function end here, without the L2 round trip.
              bool maybe = true;
              if (Q.use_occ) maybe = (occ[__mul24(t0, P.occ_roww) + (s0 >> 5)] >> (s0 & 31)) & 1u;
              col.w = 0.0f;
              if (maybe) {
                SLAB_MARK("occupancy bit");
                SLAB_FAST_ALPHA
              }
              hit = col.w != 0.0f;
            } else if (TF == 2 && Q.use_occ) {
              // dense 3-D table: the (v, g) base texel's occupancy bit, folded over the sheets (smk_set_tf3d), decides
              // whether the eight-texel gather can return anything but alpha == 0
              int s0, s1, t0, t1;
              float fs, ft;
              smk_lin_clamp(__fmaf_rn(ch0, (float)P.s3v, -0.5f), P.s3v, s0, s1, fs);
              smk_lin_clamp(__fmaf_rn(ch1, (float)P.s3g, -0.5f), P.s3g, t0, t1, ft);
              col.w = 0.0f;
              hit = false;
              if ((occ[__mul24(t0, P.occ_roww) + (s0 >> 5)] >> (s0 & 31)) & 1u) {
                SLAB_MARK("occupancy bit");
                ch2 = tri_h_early();  // (the third coordinate of the lookup: only now)
                hit = smk_classify<DT, TF>(P, ch0, ch1, ch2, ch3, col);
              }
            } else {
              SLAB_MARK("occupancy bit");  // (no bitmap: every sample goes on)
              hit = smk_classify<DT, TF>(P, ch0, ch1, ch2, ch3, col);
            }
            d_hit = hit;
            if (hit) {
              SLAB_SHOW
            }
          }
#undef SLAB_SHOW
#undef SLAB_FAST_ALPHA
          SLAB_MARK("blend");
          if (count && d_maybe) d_vis = (unsigned)__builtin_amdgcn_s_memtime() - d_t0;
#undef QI
        }
        if (act) {
          m = m_next;
          if constexpr (EARLY) {
            // (the next sample's slice was worked out when the ring slots were released; m1 may since have shrunk to m - 1
            //  -- the ray saturated -- which ends it)
            if (m <= m1) {
              car_sc = early_nsc;
              car_i = early_ni;
              pb = __mul24(psgn, car_i) + poff;
            } else pb = SLAB_DONE;
          } else if (m <= m1) {
            car_i = base_slice_c(m, car_sc);
            pb = __mul24(psgn, car_i) + poff;
          } else pb = SLAB_DONE;
        }
        if (count) {
          n_it += 1.f;
          n_act += (float)__popcll(__ballot(act));
          n_in += (float)__popcll(__ballot(work));  // lanes that interpolate a sample (an empty layer's are skipped before that)
          n_hit += (float)__popcll(__ballot(d_hit));
          n_anyhit += __any(d_hit) ? 1.f : 0.f;
          n_work += __any(work) ? 1.f : 0.f;
          n_own += __any(work && d_own) ? 1.f : 0.f;
          const unsigned long long mm = __ballot(d_maybe);
          if (mm) {  // (the stamps are the wave's: any lane that ran the visible path holds them)
            const int src = __ffsll(mm) - 1;
            n_anymaybe += 1.f;
            c_vis += (float)(unsigned)__builtin_amdgcn_readlane((int)d_vis, src);
            c_texwait += (float)(unsigned)__builtin_amdgcn_readlane((int)d_wait, src);
          }
        }
        }  // rep
        SLAB_MARK("loop tail");
      }
      if (lane == 0) lds_st(&ctl[8 + wave], SLAB_DONE);
      if (tracing && lane == 0) atomicAdd(Q.trace + 8 * (size_t)blockIdx.x + 7, (unsigned)n_it);
      if (count && lane == 0) {
        atomicAdd(&Q.diag[0], n_it);
        atomicAdd(&Q.diag[1], n_act);
        atomicAdd(&Q.diag[2], n_in);
        atomicAdd(&Q.diag[3], n_hit);
        atomicAdd(&Q.diag[8], n_anyhit);
        atomicAdd(&Q.diag[14], n_work);
        atomicAdd(&Q.diag[15], n_own);
        atomicAdd(&Q.diag[9], n_lead);
        atomicAdd(&Q.diag[10], n_waits);
        atomicAdd(&Q.diag[11], n_wstep);
        // (how much of the tile's slice range this wave did not need: it finished at position `pos`)
        atomicAdd(&Q.diag[12], (float)max(npos - min(pos, npos), 0) / (float)max(npos, 1));
        atomicAdd(&Q.diag[13], 1.0f);
        atomicAdd(&Q.diag[16], n_anymaybe);
        atomicAdd(&Q.diag[17], c_vis * 1e-3f);
        atomicAdd(&Q.diag[18], c_texwait * 1e-3f);
      }
    }
  }
  if (live) {
    size_t o = (size_t)j * P.W + i;
    float4 *outp = seg == 0 ? P.out : Q.seg_out + (size_t)(seg - 1) * ((size_t)P.W * P.H);
    outp[o] = make_float4(C0, C1, C2, C3);
    if (P.depth != nullptr && C3 == 0.0f) P.depth[o] = __int_as_float(0x7f800000);  // (no sample passed classification)
  }
  // errors are reported, never swallowed: the host turns a non-zero status into a failed frame
  if (npos > 0) {
    __syncthreads();
    if (tid == 0 && ctl[3]) *(volatile int *)Q.status = Q.status_tag | ctl[3];
  }
  if (tid == 0 && Q.tile_ticks && nseg > 1) {  // (a split tile's words are sums over its workgroups; zeroed by the launcher)
    const unsigned dur = max((unsigned)__builtin_amdgcn_s_memrealtime() - trace_t0, 1u);
    if (Q.piece_ticks) Q.piece_ticks[(size_t)tile * 8 + seg] = dur;
    atomicAdd(&Q.tile_ticks[tile], dur);
    atomicAdd(&Q.tile_ticks[Q.ntiles + tile], npos > 0 ? (unsigned)max(min(max(min(min(ctl[4], ctl[5]), min(ctl[6], ctl[7])), 0), npos + 1) - ctl[2], 0) : 0u);
    atomicAdd(&Q.tile_ticks[2 * Q.ntiles + tile], npos > 0 ? (unsigned)(npos + 1) : 0u);
  } else if (tid == 0 && Q.tile_ticks) {
    Q.tile_ticks[tile] = max((unsigned)__builtin_amdgcn_s_memrealtime() - trace_t0, 1u);
    // (ctl[4..7] = the loaders' landed words, final after the barrier above; their minimum = slices completely streamed)
    // (less the slices that were not streamed because nobody samples them: EMPTY LAYERS)
    Q.tile_ticks[Q.ntiles + tile] = npos > 0 ? (unsigned)max(min(max(min(min(ctl[4], ctl[5]), min(ctl[6], ctl[7])), 0), npos + 1) - ctl[2], 0) : 0u;
    Q.tile_ticks[2 * Q.ntiles + tile] = npos > 0 ? (unsigned)(npos + 1) : 0u;
    // (the product's own timeline, read by smk_get_trace when no diagnostic instance ran: when the workgroup started, and where)
    Q.tile_ticks[3 * Q.ntiles + tile] = trace_t0;
    Q.tile_ticks[4 * Q.ntiles + tile] = (__builtin_amdgcn_s_getreg((31 << 11) | 4) & 0xff00u) | (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xfu);
  }
  if (tracing && tid == 0) {
    unsigned *t = Q.trace + 8 * (size_t)blockIdx.x;
    if (phases) {  // 100 MHz ticks since the workgroup started: slice range known | windows tabled | flags, runs, last barrier
      t[4] = ph1;
      t[5] = ph2;
      t[6] = ph3;
    }
    t[0] = trace_t0;
    t[1] = (unsigned)__builtin_amdgcn_s_memrealtime();
    t[2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
    t[3] = (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xf) | ((unsigned)tile << 8) | ((unsigned)max(npos, 0) << 20);  // XCC_ID, tile, slices
  }
}

// ------------------------------------------------------------------------------- host side

// This file is compiled eight times, -DSLAB_PART=0..7 (build time: the instances are most of it).  Each part holds the
// instances slab_inst_part (smk_slab.h) gives it and the dispatch over them; part 0 has the merge pass and the launcher too.
#ifndef SLAB_PART
#define SLAB_PART 0
#endif
#if SLAB_PART == 0
// DEPTH SEGMENTS, second half: the partial frames of a split tile, merged in marching order.  `list` entries: tile | segments << 20.
__global__ __launch_bounds__(256) void smk_k_slab_merge(const int2 *list, int tw, int th, int ntx, int W, int H, const float4 *seg_out, float4 *out, int use_max) {
  const int code = list[blockIdx.x].x;
  const int tile = code & 0xfffff, nseg = code >> 20;
  const int ty = tile / ntx, tx = tile - ty * ntx;
  const size_t npix = (size_t)W * H;
  for (int p = threadIdx.x; p < tw * th; p += blockDim.x) {
    const int i = tx * tw + p % tw, j = ty * th + p / tw;
    if (i >= W || j >= H) continue;
    const size_t o = (size_t)j * W + i;
    float4 C = out[o];
    for (int k = 1; k < nseg; ++k) {
      const float4 sgm = seg_out[(size_t)(k - 1) * npix + o];
      if (use_max) {
        C = make_float4(fmaxf(C.x, sgm.x), fmaxf(C.y, sgm.y), fmaxf(C.z, sgm.z), fmaxf(C.w, sgm.w));
      } else {
        const float w = 1.0f - C.w;
        C.x = __fmaf_rn(w, sgm.x, C.x);
        C.y = __fmaf_rn(w, sgm.y, C.y);
        C.z = __fmaf_rn(w, sgm.z, C.z);
        C.w = __fmaf_rn(w, sgm.w, C.w);
      }
    }
    out[o] = C;
  }
}
hipError_t smk_slab_merge(const int2 *list, int n, int tw, int th, int ntx, int W, int H, const float4 *seg_out, float4 *out, int use_max,
                          hipStream_t s) {
  hipLaunchKernelGGL(smk_k_slab_merge, dim3(n), dim3(256), 0, s, list, tw, th, ntx, W, H, seg_out, out, use_max);
  return hipGetLastError();
}
// launch the instance k names, through the part that holds it
hipError_t smk_slab_launch_instance(const SlabInst &k, const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks, const char **why,
                                    hipStream_t s) {
  static SlabDispatchPart *const part[8] = {smk_slab_dispatch_part0, smk_slab_dispatch_part1, smk_slab_dispatch_part2, smk_slab_dispatch_part3,
                                            smk_slab_dispatch_part4, smk_slab_dispatch_part5, smk_slab_dispatch_part6, smk_slab_dispatch_part7};
  if ((*why = slab_inst_missing(k))) return hipErrorNotSupported;
  return part[slab_inst_part(k)](k, P, Q, lds, nblocks, s);
}
#endif  // SLAB_PART == 0

template <int DT, int SH, int PERM, int NW, int NL, bool DIAG, int TF = 1, bool BR = true, bool SHD = false, bool OCC = false, bool NVL = false>
static hipError_t launch_slab(const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks, hipStream_t s) {
  auto k = smk_k_slab<DT, SH, PERM, NW, NL, DIAG, TF, BR, SHD, OCC, NVL>;
  static bool attr_set[64] = {};  // per device: the attribute belongs to the function ON the current device
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  hipLaunchKernelGGL(k, dim3(nblocks), dim3((NW + NL) * 64), lds, s, P, Q);
  return hipGetLastError();
}

// ---- instance dispatch (declared in smk_slab.h).  Every key of the cross product is visited: slab_inst_at(I, F), F over
// the flags, I over voxels x shading x axis x shape x table.  A key that is built and belongs to this part becomes a
// comparison with the run-time key and a launch; any other key becomes nothing -- the discarded branch of an `if constexpr`
// on the template's own parameters instantiates no kernel.
constexpr bool slab_inst_here(SlabInst K) { return !slab_inst_missing(K) && slab_inst_part(K) == SLAB_PART; }
template <int I, int F>
static bool slab_try(const SlabInst &k, const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks, hipStream_t s, hipError_t *e) {
  constexpr SlabInst K = slab_inst_at(I, F);
  if constexpr (slab_inst_here(K)) {
    if (k == K) {
      *e = launch_slab<K.dt, K.sh, K.perm, K.nw, K.nl, K.diag, K.tf, K.br, K.shd, K.occ, K.nvl>(P, Q, lds, nblocks, s);
      return true;
    }
  }
  return false;
}
// (two folds, one inside the other: a single fold over all the keys is deeper than the compiler nests an expression.  The
//  flags are the outer one: most of their 32 combinations have no key in this part and are passed over whole -- build time)
template <int F, int... I>
static bool slab_try_kinds(std::integer_sequence<int, I...>, const SlabInst &k, const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks,
                           hipStream_t s, hipError_t *e) {
  if constexpr ((slab_inst_here(slab_inst_at(I, F)) || ...)) return (slab_try<I, F>(k, P, Q, lds, nblocks, s, e) || ...);
  return false;
}
template <int... F>
static bool slab_try_all(std::integer_sequence<int, F...>, const SlabInst &k, const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks,
                         hipStream_t s, hipError_t *e) {
  return (slab_try_kinds<F>(std::make_integer_sequence<int, SLAB_INST_KINDS>{}, k, P, Q, lds, nblocks, s, e) || ...);
}
#define SLAB_PASTE_(a, b) a##b
#define SLAB_PASTE(a, b) SLAB_PASTE_(a, b)
hipError_t SLAB_PASTE(smk_slab_dispatch_part, SLAB_PART)(const SlabInst &k, const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks,
                                                         hipStream_t s) {
  hipError_t e = hipErrorNotSupported;  // (a key of another part, or one that is not built: smk_slab_launch_instance sends neither)
  slab_try_all(std::make_integer_sequence<int, SLAB_INST_FLAGS>{}, k, P, Q, lds, nblocks, s, &e);
  return e;
}
