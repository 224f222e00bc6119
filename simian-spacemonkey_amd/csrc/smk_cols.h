// smk_cols.h -- what the column-stream kernel (smk_cols.hip) and its planner (smk_cols_plan.hip) both know: the launch
// parameters, the job limits, the workgroup shapes and the launches the planner makes.
#pragma once

#include "smk_internal.h"

#define COL_DONE 0x3fffffff
#define COL_MAX_CL 256      // positions per job at most (the per-slice table lives in LDS)
#define COL_MAX_RAYS 4096   // rays one job can list (8 bytes each in LDS)
#define COL_BOX_MARGIN 0.05f
#define COL_LDS_CAP (160 * 1024)  // dynamic LDS of one workgroup at most

// wave-uniform description of one launch
struct ColParams {
  const char *lay;            // layout base: [cv][cu][s][(CH+1)][(CW+1)] voxels, slice images of slice_bytes
  int CW, CH, ncu, ncv;       // cells per column along U, V; columns
  int Ou, Ov, Os;             // stored-box origin (global voxel index) along U, V, S
  int Du, Dv, Ds;             // stored-box dims
  int slice_bytes;            // (CW+1)(CH+1) voxels, rounded up to 16 bytes
  int n_ch;                   // DMA wave-instructions per slice = ceil(slice_bytes / 1024)
  unsigned long long last_mask;  // lanes of the last one
  int nslots, maxfly, wstep;
  int take_min, take_wait;    // a wave takes new rays when this many lanes are free, or after this many turns
  int ring_bytes;             // LDS bytes in front of the tables: the ring, at least the set-up's scratch (the unsorted rays)
  int CL, nck;                // positions per chunk, chunks
  int dir;                    // +1: rays advance towards +S
  float Mx[4], My[4], Mw[4];  // voxel (global coordinates) -> continuous pixel: x = Mx.(X,1) / Mw.(X,1)
  float4 *layers;             // [nkeys][npix]
  unsigned long long *masks;  // [npix][mask_words]
  int nkeys, mask_words;
  int use_ah, use_occ, fast_tf;
  int *status;                // host-visible: status_tag | (1 protocol time-out, 3 a job's rays do not fit lanes or list, 5 a ray's plane count
                              // does not fit its list entry)
  int status_tag;             // the frame's id << 8
  unsigned *job_ticks;        // [njobs] duration of each job's workgroup in 100 MHz ticks, or null
  unsigned long long *counts; // [8] samples taken | visible | slices streamed | segments written | consumer wave-iterations | lanes with a sample to
                              // take in them | iterations in which some lane changes rays | lanes changing rays (developer statistics)
};

// workgroup shapes: {consumer waves, loader waves}; option cols_shape k picks entry k - 1
struct ColShape { int nw, nl; };
static const ColShape kColShapes[] = {{15, 1}, {14, 2}};
constexpr int COL_NSHAPES = (int)(sizeof kColShapes / sizeof kColShapes[0]);

// ---- the launches (smk_cols.hip, where the kernel's instances live; hidden: not part of the library's interface)
#pragma GCC visibility push(hidden)
// the column layout of the native [z][y][x] stored box for layout perm (ColLayout), `blocks` workgroups of 256 threads
hipError_t smk_cols_build(const void *vox_native, int dtype, int perm, const int D[3], int CW, int CH, int ncu, int ncv, int slice_bytes,
                          void *dst, unsigned blocks, hipStream_t s);
// the marching kernel's instance for the mode, layout perm and workgroup shape; hipErrorInvalidValue where none exists
hipError_t smk_cols_march(const RenderParams &P, const ColParams &Q, int dtype, int tf_mode, int shade_kind, int perm, int shape, size_t lds,
                          int njobs, hipStream_t s);
// the resolve pass: every pixel's segments blended in key order (maximum with use_max), the masks cleared
hipError_t smk_cols_resolve(const float4 *layers, unsigned long long *masks, int mask_words, size_t npix, float4 *out, int use_max,
                            hipStream_t s);
#pragma GCC visibility pop
