// smk_slab.h -- what the slice-ring kernel (smk_slab.hip) and its planner (smk_slab_plan.hip) both know: the launch
// parameters, the slice-table entry, the workgroup classes and the instance dispatch.
#pragma once

#include "smk_internal.h"

// wave-uniform description of one launch
struct SlabParams {
  int perm;                    // 0: S=z (U=x,V=y)  1: S=y (U=x,V=z)  2: S=x (U=y,V=z; x-major copy)
  int au, av, as;              // model-axis index of U, V, S
  long long strideV, strideS;  // voxel strides of the layout in use (U stride is 1)
  int Ou, Ov, Os;              // stored-box origin along U,V,S (global voxel index)
  int Du, Dv, Ds;              // stored-box dims along U,V,S
  int wu;                      // 16-byte units per window row that are loaded at most (<= wp)
  int wv;                      // window rows that are loaded
  int wp;                      // LDS row pitch in 16-byte units, a multiple of 8: the slot image is flat with this
                               // pitch, so the (row, column) a DMA lane serves repeats every `per` chunks = `rpg` rows
  int per, rpg;                // chunks and rows per group: per = wp / gcd(64, wp), rpg = 64 / gcd(64, wp)
  int groups;                  // row groups per slice = ceil(wv / rpg); chunks = groups * per
  int mask_need;               // loaders fetch only what each slice needs of the window (big windows)
  int chunks;                  // DMA wave-instructions per slice = ceil(wv / rows per chunk), uniform
  int slot_bytes;              // chunks * 1024
  int nslots;                  // ring size
  int maxfly;                  // slices a loader keeps in flight ((maxfly-1) * its chunks <= 63)
  int wstep;                   // a wave steps when slices up to its slowest lane's position + 1 + wstep have landed
  int pmask;                   // consumers publish progress when (iteration & pmask) == 0
  int dir;                     // +1: rays advance towards +S, -1: towards -S
  int tw, th;                  // pixel tile
  const void *vox;             // layout base (native or x-major)
  int use_ah;                  // third-axis alpha served from a 1-D LDS table (<= 3 channels)
  int use_occ;                 // (V,G) occupancy bitmap copied to LDS
  int fast_tf;                 // alpha-first classification with 8-byte texel loads (no third axis, or use_ah)
  const unsigned char *bricks;  // brick flags of the stored box (smk_bricks.hip) or null: see "EMPTY LAYERS" in the kernel
  int bsu, bsv, bss;           // their strides along U, V, S (in bricks)
  const int2 *order;           // workgroup of each block: {tile | piece << 20 | pieces << 26, cut fractions lo | hi << 8} (work-balanced
                               // schedule, .x = -1: none), see slab_schedule and DEPTH SEGMENTS
  unsigned *tile_ticks;        // [5][ntiles]: duration of each tile's workgroup in 100 MHz ticks (next frame's weights) |
                               // slices its loaders streamed | slices of its range (the loaders stop once every ray of
                               // the tile is saturated: what was NOT streamed is not counted as read, smk_last_frame_info)
  int ntiles;
  int *status;                 // host-visible word: status_tag | (1 = protocol time-out, 2 = window bound violated)
  int status_tag;              // the frame's id << 8: a word written late, into a slot that has been handed on, is told apart by it
  float *diag;                 // [16] diagnostic counters (lockstep bit 16) or null
  unsigned *trace;             // [nblocks][8] per-workgroup timeline record (lockstep bit 32, see smk.h) or null
  float4 *seg_out;             // [maxseg - 1][W * H]: partial frames of the depth segments 1.. of split tiles (DEPTH SEGMENTS), or null
  unsigned *piece_ticks;       // [ntiles][8]: duration of every piece of a split tile (where the next cuts come from)
};

// per-slice table entry: where the slice's window sits in the ring and in the volume
struct SlabEnt {
  int base;      // LDS byte address of GLOBAL voxel (u=0, v=0) of this slice's slot image:
                 // corner address = base + v * pitch_bytes + u * voxel_bytes
  unsigned pack;  // loader: window origin u0 | v0 << 11 (stored-box voxels), (units the slice needs - 1) << 22,
                  // rows of the window the slice can spare, in sixteenths of wv, << 28
};

// slack of the window bounds against the kernels' fp32 coordinate chains
#define SLAB_EPS 0.02f

// workgroups of more waves than this are "big": one per CU
constexpr int SLAB_BIG_WAVES = 12;
constexpr bool slab_big(int nw, int nl) { return nw + nl > SLAB_BIG_WAVES; }
// The loaders form NLG groups; group g streams slices g, g + NLG, ... and its loaders share the row groups of each.  Small
// workgroups: a loader per slice.  Big ones, whose ring is too short for NL slices filled at once: two groups (or one).
constexpr int SLAB_BIG_NLG = 2;
constexpr int slab_loader_groups(int nw, int nl) { return slab_big(nw, nl) ? ((nl % SLAB_BIG_NLG) == 0 ? SLAB_BIG_NLG : 1) : nl; }

// ---- instance dispatch, one function per voxel type (one translation unit each); hipErrorNotSupported and *why where
// no instance exists
hipError_t smk_slab_dispatch_u8(const RenderParams &P, const SlabParams &Q, int tf_mode, int shade_kind, int nw, int nl, bool diag, size_t lds,
                                int nblocks, const char **why, hipStream_t s);
hipError_t smk_slab_dispatch_f32(const RenderParams &P, const SlabParams &Q, int tf_mode, int shade_kind, int nw, int nl, bool diag, size_t lds,
                                 int nblocks, const char **why, hipStream_t s);
// u16 voxels (SMK_U16: 8-byte voxels, staged like the u8 ones, their own corner decode): the plain instances and the eye pass
// of frames with shadows under look 0.  Left unbuilt, and declined by slab_refusal with the reason: the instances for the
// host's scene depth and for the NV20 look -- the gather kernel renders those frames
hipError_t smk_slab_dispatch_u16(const RenderParams &P, const SlabParams &Q, int tf_mode, int shade_kind, int nw, int nl, bool diag, size_t lds,
                                 int nblocks, const char **why, hipStream_t s);
hipError_t smk_slab_dispatch_u16_shadow(const RenderParams &P, const SlabParams &Q, int tf_mode, int shade_kind, int nw, int nl, size_t lds,
                                        int nblocks, const char **why, hipStream_t s);
// ... and the u16 instances that are NOT built because they would need scratch: NV20 shading under the dense 3-D table, 10+2
// waves, brick flags -- at the 80 VGPRs of their launch bound they spill 6 (the u8 counterparts, which exist, spill 1).  One
// predicate for the dispatch and for the shape choice, as slab_nv20_left_out below
constexpr bool slab_u16_left_out(int dtype, int shade_kind, int tf_mode, int nw, int nl, bool bricks) {
  return dtype == 2 && shade_kind == 2 && tf_mode == 2 && nw == 10 && nl == 2 && bricks;
}
constexpr const char *SLAB_U16_LEFT_OUT = "u16 voxels have no 10+2-wave instances with NV20 shading, the 3-D table and brick flags (they would spill)";
constexpr const char *SLAB_U16_NO_OCC = "u16 voxels have no scene-depth instances of the slice-ring kernel";
constexpr const char *SLAB_U16_NO_NV20 = "u16 voxels have no shadow_look 1 instances of the slice-ring kernel";
// ... and one for the eye pass of frames with shadows (SHD instances: 2-D / 3-D table, R8k shading or none, u8 and f32 voxels)
hipError_t smk_slab_dispatch_shadow(const RenderParams &P, const SlabParams &Q, int dtype, int tf_mode, int shade_kind, int nw, int nl, size_t lds,
                                    int nblocks, const char **why, hipStream_t s);
// The NV20 look's slice-ring instances that are NOT built: float voxels, 10+2 waves, brick flags -- at the 80 VGPRs of their
// launch bound they would spill (profiles/shadow_nv20.md).  One predicate for the dispatch, which declines such a launch, and
// for the shape choice, which passes such a shape over (smk_slab_plan.hip)
constexpr bool slab_nv20_left_out(int dtype, int nw, int nl, bool bricks) { return dtype == 1 && nw == 10 && nl == 2 && bricks; }
constexpr const char *SLAB_NV20_LEFT_OUT = "option shadow_look 1 has no float-voxel 10+2-wave instances with brick flags (they would spill)";
// ... and one for that eye pass in the NV20 look (option shadow_look 1; NVL instances: shading none or NV20 Phong)
hipError_t smk_slab_dispatch_shadow_nv20(const RenderParams &P, const SlabParams &Q, int dtype, int tf_mode, int shade_kind, int nw, int nl,
                                         size_t lds, int nblocks, const char **why, hipStream_t s);
// ... and for frames with the host's opaque scene depth (OCC instances, smk_render_occluded): view-aligned planes, and the eye
// pass of frames with shadows
hipError_t smk_slab_dispatch_occluded(const RenderParams &P, const SlabParams &Q, int dtype, int tf_mode, int shade_kind, int nw, int nl, size_t lds,
                                      int nblocks, const char **why, hipStream_t s);
hipError_t smk_slab_dispatch_occluded_shadow(const RenderParams &P, const SlabParams &Q, int dtype, int tf_mode, int shade_kind, int nw, int nl,
                                             size_t lds, int nblocks, const char **why, hipStream_t s);
// DEPTH SEGMENTS: the merge pass over the n split tiles listed at `list` (tile | pieces << 20)
hipError_t smk_slab_merge(const int2 *list, int n, int tw, int th, int ntx, int W, int H, const float4 *seg_out, float4 *out, int use_max,
                          hipStream_t s);
