// smk_slab.h -- what the slice-ring kernel (smk_slab.hip) and its planner (smk_slab_plan.hip) both know: the launch
// parameters, the slice-table entry, the workgroup classes, and the kernel's instances: their key, which of them are built,
// and their launch.
#pragma once

#include <utility>

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

// ---- instances of smk_k_slab<DT, SH, PERM, NW, NL, DIAG, TF, BR, SHD, OCC, NVL> (DESIGN.md "Instances of the slice-ring
// kernel").  One key names an instance; slab_inst_missing is the ONLY statement of which keys are built -- the build
// (smk_slab.hip compiles exactly the keys of its part), the dispatch and the planner's refusals all ask it.
struct SlabInst {
  int dt, sh, perm, nw, nl, tf;  // voxels u8 / f32 / u16 | shading none / R8k / NV20 | slice axis | consumer + loader waves | 1-D / 2-D / 3-D table
  bool diag, br, shd, occ, nvl;  // developer counters | brick-flag code | eye pass of a frame with shadows | host's scene depth | NV20 look
};
constexpr bool operator==(const SlabInst &a, const SlabInst &b) {
  return a.dt == b.dt && a.sh == b.sh && a.perm == b.perm && a.nw == b.nw && a.nl == b.nl && a.tf == b.tf && a.diag == b.diag && a.br == b.br &&
         a.shd == b.shd && a.occ == b.occ && a.nvl == b.nvl;
}
constexpr int SLAB_SHAPES[3][2] = {{8, 2}, {10, 2}, {12, 4}};  // 32x16 px | 40x16 or 16x40 px | 32x24 px and the shapes of option "tile"
// the domain: voxels x shading x axis x shape x table (i) x the five flags (f)
constexpr int SLAB_INST_KINDS = 3 * 3 * 3 * 3 * 3, SLAB_INST_FLAGS = 32;
constexpr SlabInst slab_inst_at(int i, int f) {
  return {i / 81, i / 27 % 3, i / 9 % 3, SLAB_SHAPES[i / 3 % 3][0], SLAB_SHAPES[i / 3 % 3][1], i % 3,
          (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, (f & 8) != 0, (f & 16) != 0};
}
constexpr const char *SLAB_U16_LEFT_OUT = "u16 voxels have no 10+2-wave instances with NV20 shading, the 3-D table and brick flags (they would spill)";
constexpr const char *SLAB_U16_NO_OCC = "u16 voxels have no scene-depth instances of the slice-ring kernel";
constexpr const char *SLAB_U16_NO_NV20 = "u16 voxels have no shadow_look 1 instances of the slice-ring kernel";
constexpr const char *SLAB_NV20_LEFT_OUT = "option shadow_look 1 has no float-voxel 10+2-wave instances with brick flags (they would spill)";
constexpr const char *SLAB_NV20_NO_OCC = "option shadow_look 1 has no scene-depth instances of the slice-ring kernel";
// nullptr: the instance is built; else why not (the text a declined frame reports)
constexpr const char *slab_inst_missing(SlabInst k) {
  // whole frame classes, whatever the shape: the gather kernel renders them
  if (k.dt == 2 && k.occ) return SLAB_U16_NO_OCC;
  if (k.dt == 2 && k.nvl) return SLAB_U16_NO_NV20;
  if (k.nvl && k.occ) return SLAB_NV20_NO_OCC;
  const bool plain = !k.shd && !k.occ && !k.nvl;
  const char *none = k.nvl ? "no shadow_look 1 instance for this configuration"
                   : k.occ ? "no scene-depth instance for this configuration"
                   : k.shd ? (k.dt == 2 ? "no u16 shadow instance for this configuration" : "no shadow instance for this configuration")
                           : "no kernel instance for this tile size";
  bool shape = false;
  for (const auto &s : SLAB_SHAPES) shape = shape || (k.nw == s[0] && k.nl == s[1]);
  if (!shape && plain && k.tf == 2) return "no dense-3-D-table instance for this tile size";
  if (!shape || k.dt < 0 || k.dt > 2 || k.sh < 0 || k.sh > 2 || k.perm < 0 || k.perm > 2 || k.tf < 0 || k.tf > 2) return none;
  if (k.nvl && !k.shd) return none;  // (the look is a property of the eye pass)
  // developer counters: float voxels with R8k shading under the 2-D table only, with the brick-flag code
  if (k.diag) return k.dt == 1 && k.sh == 1 && k.tf == 1 && k.br && plain ? nullptr : none;
  // shading: the eye pass shades R8k under look 0, NV20 under the NV20 look
  if (k.shd && k.sh == (k.nvl ? 1 : 2)) return none;
  if (k.shd && k.tf == 0) return "shadows need a 2-D or 3-D table";
  // the 1-D colour table: unshaded (the scalar renderer does not shade), and it has no brick flags
  if (k.tf == 0 && k.sh != 0) return k.occ ? "no colour-table instance with this shading" : "no colour-table instance for this tile size";
  if (k.tf == 0 && k.br) return none;
  // scene depth: under a 2-D / 3-D table always with the brick-flag code (it is exact with no flags)
  if (k.occ && k.tf != 0 && !k.br) return none;
  // left out because they would need scratch at the 80 VGPRs of the 10+2-wave launch bound, with the brick-flag code: the
  // NV20 look's float-voxel instances (they would spill 1-4 VGPRs, profiles/shadow_nv20.md) and the plain u16 ones with NV20
  // shading under the 3-D table (6 VGPRs; the u8 counterparts, which exist, spill 1; profiles/u16.md)
  if (k.nw == 10 && k.nl == 2 && k.br && k.nvl && k.dt == 1) return SLAB_NV20_LEFT_OUT;
  if (k.nw == 10 && k.nl == 2 && k.br && plain && k.dt == 2 && k.sh == 2 && k.tf == 2) return SLAB_U16_LEFT_OUT;
  return nullptr;
}
// The translation unit that holds an instance (the instances are most of the library's build time, so smk_slab.hip is
// compiled eight times, -DSLAB_PART=n): 0 u8, 1 f32, 6 u16 voxels, plain frames (part 0 has the merge pass and the launcher
// too, part 1 the diagnostic instances) | 2, 7 the eye pass of frames with shadows, u8 + f32 and u16 | 3, 4 scene depth
// without and with shadows | 5 the eye pass in the NV20 look
constexpr int slab_inst_part(SlabInst k) { return k.nvl ? 5 : k.occ ? (k.shd ? 4 : 3) : k.shd ? (k.dt == 2 ? 7 : 2) : k.dt == 2 ? 6 : k.dt; }
// launch the instance k names: hipErrorNotSupported and *why = slab_inst_missing's reason where it is not built
hipError_t smk_slab_launch_instance(const SlabInst &k, const RenderParams &P, const SlabParams &Q, size_t lds, int nblocks, const char **why,
                                    hipStream_t s);
// ... through the part that holds it: each translation unit of smk_slab.hip exports the dispatch over its own instances
using SlabDispatchPart = hipError_t(const SlabInst &, const RenderParams &, const SlabParams &, size_t, int, hipStream_t);
SlabDispatchPart smk_slab_dispatch_part0, smk_slab_dispatch_part1, smk_slab_dispatch_part2, smk_slab_dispatch_part3, smk_slab_dispatch_part4,
    smk_slab_dispatch_part5, smk_slab_dispatch_part6, smk_slab_dispatch_part7;
// DEPTH SEGMENTS: the merge pass over the n split tiles listed at `list` (tile | pieces << 20)
hipError_t smk_slab_merge(const int2 *list, int n, int tw, int th, int ntx, int W, int H, const float4 *seg_out, float4 *out, int use_max,
                          hipStream_t s);
