// smk_internal.h -- context and kernel-parameter structures of the HIP ray-marcher.
// Product code: never includes anything from oracle/.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/smk.h"
#include "smk_packed.h"

#define SMK_MAX_RANKS 8
#define SMK_TIMING_RING 64
#define SMK_BRICK_LOG2 3   // bricks of 8x8x8 cells (smk_bricks.hip)
#define SMK_SHADOW_BOX_EPS 0.0009765625f  // voxels: frames with shadows test eye and light samples against the box widened by this (smk_shadow_plan.hip)
#define SMK_TUNE_SETTLE 6  // auto mode: untimed slice-ring frames before a new configuration's timed trial (smk_frame.hip)
#define SMK_STATUS_RING 8  // frames whose slice-ring status stays readable (smk_frame_failed)

// error handling of the C ABI entries (int returns: 0 ok, 1 error with the message in ctx->err)
#define HIPCHK(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess) {                                                            \
      char b_[512];                                                                    \
      snprintf(b_, sizeof b_, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      (ctx)->err = b_;                                                                 \
      return 1;                                                                        \
    }                                                                                  \
  } while (0)

#define FAIL(ctx, ...)                     \
  do {                                     \
    char b_[512];                          \
    snprintf(b_, sizeof b_, __VA_ARGS__);  \
    (ctx)->err = b_;                       \
    return 1;                              \
  } while (0)

// Eye rays of a frame with shadows (half-angle slicing, smk_shadow.hip).  The slice planes are not perpendicular to the
// view axis, so a ray's coefficients are not affine in the pixel coordinate; they are (smk_ray_AB, smk_device.h)
//   D_a = fma(px, Dx_a, fma(py, Dy_a, Dc_a)),  nD = fma(px, nDx, fma(py, nDy, nDc)),
//   tauA = numA / nD, dtau = dB / nD,  A_a = fma(tauA, D_a, Ec_a),  B_a = dtau * D_a
// and plane m = 0..nplanes-1, counted FROM THE EYE, holds the sample fma(m, B, A) where fma(m, dtau, tauA) is positive and
// finite (a sample behind the eye does not exist).  Plane m is slice k = k0 + dk m of the light's order (k = 1..nslices away
// from the light); its sample is shaded under the light buffer as slices < k left it: hist[k - 1].
struct SmkShadowRays {
  int on;  // 0: the affine coefficients of smk_raycoef; 1: these, the R8k look; 2: these, the NV20 look (option shadow_look 1)
  float Ec[3], Dc[3], Dx[3], Dy[3], nDc, nDx, nDy;
  float numA, dB;
  float llo[3], lhi[3];  // the box a LIGHT ray's sample must lie in (closed): the volume, or what an orthogonal clip plane leaves of it
  int k0, dk, LB;
  float Xm[4], Ym[4], Wm[4], lscale, lbias;
  float keep;  // the NV20 look: 1 - amb, one fp32 subtraction on the host -- a fully shadowed sample keeps the fraction amb of
               // its colour (smk_shadow_keep, smk_device.h; where the pointer's alignment left four bytes: no field moves)
  const float4 *hist;  // [nslices + 1] buffers of [LB][LB] texels, `hstride` texels apart
  long long hstride;   // (LB * LB + a pad: buffers a power of two apart would meet in the same memory channels)
};
static_assert(sizeof(SmkShadowRays) == 184, "keep sits in the padding before hist: the kernarg layout of every kernel stays as it was");

// A frame with shadows on one shard of a sort-last split (smk_shadow.hip; DESIGN.md 4b, "Shadows on shards").  A texel's
// light ray ENTERS grown(j) -- rank j's region widened by its margin m_j -- at its first sample (slices k0..k1 of the whole
// volume's bracket, in the light's order) inside that box.  Phase 1: rank r marches the samples it owns and keeps, per
// destination j, the value before the entry into grown(j): X_{r->j}.  Phase 2: rank j composes E_j = the X_{r->j} in the
// light's BSP order and marches, from E_j, the unsharded samples after the entry that lie in grown(j) + 0.25 voxels.
struct SmkShadowShard {
  int nranks, rank;
  float olo[3], ohi[3];                                 // the light samples this rank owns (closed; an inner upper face one float below the split)
  float glo[SMK_MAX_RANKS][3], ghi[SMK_MAX_RANKS][3];   // grown(j) for every rank j
  float xlo[3], xhi[3];                                 // phase 2: grown(rank) + 0.25 voxels (inside region + halo when halo >= m + 1)
  int order[SMK_MAX_RANKS];                             // the ranks in the light's BSP order, nearest the light first
  const float4 *entries;                                // phase 2: [nranks][LB][LB] X_{r->rank}, r in rank order
  float4 *exports;                                      // phase 1: [nranks][LB][LB] X_{rank->j} (slot rank zero)
};

// Everything a render kernel needs, passed by value as the kernarg (wave-uniform => SGPRs).
struct RenderParams {
  // ---- volume, packed layout (DESIGN.md "HBM layout")
  //   u8 : uint2  {c0|c1<<8|c2<<16|c3<<24, n0|n1<<8|n2<<16}                 8 B/voxel
  //   f32: float4 {c0,c1,c2, c3 or normal bits}                            16 B/voxel
  const void *vox;
  const uint32_t *nrm;  // separate packed normals (only f32 with 4 channels), else null
  int N[3];             // whole-volume dims
  int O[3];             // global index of stored voxel (0,0,0)
  int D[3];             // stored dims (region + halo)
  float lo[3], hi[3];   // region in voxel coordinates: [g0-.5, g1-.5)
  int top[3];           // region touches the volume's top face on this axis (inclusive)
  int cplane_on;        // free clip plane: a sample stays when fma-chain(cplane . (p,1)) >= 0 (voxel coordinates)
  float cplane[4];
  float hin[3];         // largest coordinate that is inside: hi on a top face, else the float below hi
  float invN[3];
  int nelts;
  int n_in_w;  // f32: normal bits live in .w
  // ---- classification
  const float4 *tlut;  // premultiplied (r*a,g*a,b*a,a)
  int tlut_size;
  const uint32_t *tf_vg;  // [sg][sv] RGBA8
  const uint32_t *tf_h;   // [sg][sv] RGBA8 (alpha used) or null
  const uint32_t *tf_occ;  // [sg][occ_roww] bit s of row t: the bilinear lookup based at texel (s,t) can be non-transparent
  int occ_roww;
  int sv, sg, third_axis;
  const uint32_t *tf3d;  // [s3h][s3g][s3v]
  int s3v, s3g, s3h;
  // ---- brick flags (smk_bricks.hip): [nbr[2]][nbr[1]][nbr[0]] bytes over the stored box, 0 = no sample whose cell lies in
  // the brick can be visible under the current table; null = not available (1-D colour table, option "bricks" 0)
  const unsigned char *bricks;
  int nbr[3];
  const unsigned char *bricks_dil;  // the same, each flag spread over the bricks a perturbed fetch can reach from there, or null
  // ---- camera / sample placement
  smk_raycoef rc;
  SmkShadowRays sh;
  int W, H;
  float znear;
  // ---- shading
  int use_spec;
  float L[3], Hv[3];
  float R[9];  // rows of rinfo.xform's rotation: Nw = R * n
  float intens;
  int blend;  // smk_blend
  // ---- perturbation
  const uint32_t *noise;  // [nn][nn][nn] RGBA8
  int nn, pert_on;
  int nn_log2;  // log2(nn) when the noise texture's edge is a power of two, else -1
  float pw[2], ps[2];
  // ---- output
  float4 *out;
  float *depth;
  // ---- tile mapping
  int ntx, nty, tiles_per_xcd;
  int wave_w, blk_w, lockstep;  // gather-kernel tiling knobs (smk_set_option)
  // ---- the host's opaque scene depth (smk_render_occluded): [H][W] floats of the window, or null.  A sample exists only
  // where its smk_plane_depth is less than the pixel's smk_scene_depth (smk_device.h); kind = smk_scene_depth_kind, and
  // for window depths zs_fn = f n, zs_f = f, zs_fmn = f - n of the camera's clip planes.  (Last: the fields above keep
  // their kernarg offsets, and the kernels without a scene depth their register allocation.)
  const float *zscene;
  int zscene_kind;
  double zs_fn, zs_f, zs_fmn;
};

// side buffers of the slice-ring kernel, owned by the context
constexpr int SMK_SLAB_NDIAG = 19;  // counters of the slice-ring kernel's diagnostic instance (names: smk_get_stat)
struct SlabAux {
  int *h_status = nullptr;      // pinned, device-visible: SMK_STATUS_RING error words (0 = ok), one per frame in turn
  int status_slot = 0;          // the word of the frame being launched
  int status_tag = 0;           // ... and that frame's id << 8, which the kernel writes with its status
  hipEvent_t frame_ev0 = nullptr;  // recorded by the launcher right before its first stream operation
  float *d_diag = nullptr;      // [SMK_SLAB_NDIAG] diagnostic counters (option lockstep bit 16)
  int2 *d_order = nullptr;      // workgroup schedule of the current camera
  int2 *h_order[4] = {nullptr, nullptr, nullptr, nullptr};  // pinned staging copies, used in turn
  hipEvent_t order_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // completion of each one's last copy
  int order_next = 0;
  int order_cap = 0;
  std::vector<int2> order_host;  // what d_order holds
  struct Scan {  // the per-tile geometry scan of the last frame, per workgroup configuration tried (key = camera + region + tile shape)
    std::vector<unsigned char> key;
    double v[4] = {0, 0, 0, 0};
    std::vector<int> work;
    int slices = 0;  // load indices (npos + 1) of the longest tile
  } scan[4];
  unsigned scan_next = 0;
  std::vector<unsigned char> shape_key;  // the small-workgroup shape chosen for this view class (see the launcher's probing pass)
  int shape_choice = -1, shape_age = 0, shape_chunks = 0;  // (... its age in frames, and the DMA chunks per slice it had when chosen)
  std::vector<int> plan_work;   // the weights the last schedule was built from,
  std::vector<unsigned char> plan_cuts;  // the cuts,
  std::vector<int2> plan_order;  // and that schedule
  int plan_slots = 0;
  // per-tile workgroup durations of an earlier frame: the schedule's weights
  unsigned *d_ticks = nullptr, *h_ticks = nullptr;  // device buffer the kernel writes; pinned copy in flight
  int ticks_cap = 0, ticks_pending_n = 0, ticks_age = 0, ticks_adopted = 0;
  int ticks_n_last = 0;  // tiles of the latest slice-ring launch (d_ticks holds [3][that many] words)
  bool ticks_pending = false;
  long long ticks_pending_sig = 0, ticks_good_sig = -1;
  hipEvent_t ticks_ev = nullptr;
  std::vector<unsigned> ticks_good;
  // DEPTH SEGMENTS (smk_slab.hip): partial frames of the pieces 1.. of split tiles, [maxseg - 1][W * H] float4
  void *d_seg = nullptr;
  size_t seg_cap = 0;
  int opt_split = 0;            // option "slab_split": 0 auto, 1 off, 2.. forced
  // developer options (0 = the planner decides): "tile" (workgroup shape id), "slab_T" (band wait + 1), "slab_fly"
  // (slices a loader keeps in flight), "slab_ns" (cap on the ring's slots)
  int opt_tile = 0, opt_T = 0, opt_fly = 0, opt_ns = 0;
  bool ticks_stale = false;     // the copy in flight measured another time step: dropped when it arrives
  int nsplit_last = 0, nblocks_last = 0;
  std::vector<unsigned char> ksplit_last;  // pieces per tile of the latest launch
  unsigned *d_pticks = nullptr, *h_pticks = nullptr;  // [ntiles][8] durations of the pieces of split tiles (device; pinned copy)
  std::vector<unsigned> pticks_good;                   // the latest that came back ...
  std::vector<unsigned char> cuts, cuts_pending, cuts_good;  // [ntiles][10] {K, cut_0..cut_K}: current | of the copy in flight | of pticks_good
  int cuts_split = -1;
  long long cuts_sig = -1;
  bool recut = true, cuts_engaged = false, merge_warm = false;
  unsigned *d_trace = nullptr;  // [trace_n][8] workgroup timeline of the last traced frame (option lockstep bit 32)
  int trace_cap = 0, trace_n = 0;
  // the plan of the latest slice-ring launch, host-side (smk_get_stat "slab_plan_*", smk_slab_plan.hip): SlabParams'
  // window, pitch, ring and flag fields, the workgroup shape and its LDS bytes, the most DMA instructions one loader
  // issues per slice, and the slices of the longest tile (scan_slices: of the latest window scan)
  static constexpr int PLAN_FIELDS = 25;
  int plan_last[PLAN_FIELDS] = {0};
  int scan_slices = 0;
};

// the column-stream kernel's side buffers (smk_cols_plan.hip), owned by the context
struct ColLayout {  // the stored box re-laid out for one principal axis: [cv][cu][s][(CH+1)][(CW+1)] voxels
  void *d = nullptr;
  size_t bytes = 0;
  int CW = 0, CH = 0, ncu = 0, ncv = 0, Du = 0, Dv = 0, Ds = 0, slice_bytes = 0, vb = 0;
  const void *src = nullptr;  // the native volume it was built from
};
struct ColsAux {
  ColLayout lay[3];             // per principal axis (perm 0: S = z, 1: S = y, 2: S = x), built on first use
  void *d_layers = nullptr;     // [nkeys][npix] float4: a ray's partial composites, one per job it crosses
  size_t layers_cap = 0;
  void *d_masks = nullptr;      // [npix][mask_words] bit per key written
  size_t masks_cap = 0;
  bool masks_dirty = true;
  int mask_words_last = 0;
  unsigned *d_ticks = nullptr;  // [njobs] workgroup durations of the latest frame (100 MHz ticks)
  int ticks_cap = 0, njobs_last = 0;
  unsigned long long *d_counts = nullptr;  // [8] developer statistics of the latest frame (ColParams::counts)
  int want_counts = 0;
  // developer knobs (smk_set_option cols_shape, cols_ns, cols_chunk, cols_wstep, cols_fill, cols_take_min, cols_take_wait,
  // cols_fly; 0 = the planner decides)
  int opt_shape = 0, opt_ns = 0, opt_chunk = 0, opt_wstep = 0;
  int opt_fill = 0, opt_take_min = 0, opt_take_wait = 0, opt_fly = 0;
  int builds = 0;               // layouts built so far
  int cw_last = 0, ch_last = 0, nslots_last = 0, shape_last = 0;  // columns, ring slots and workgroup shape of the latest launch
  double last_stream_bytes = 0; // bytes the loaders of the latest launch had to stream
  // the launch plan of the latest launch (smk_get_stat "cols_plan_<field>", smk.h; the order of kColsPlanFields in
  // smk_cols_plan.hip)
  static constexpr int PLAN_FIELDS = 19;
  int plan_last[PLAN_FIELDS] = {0};
  hipEvent_t frame_ev0 = nullptr;
  int status_tag = 0;           // the frame's id << 8 (written with a status word)
};
void smk_cols_free(ColsAux *aux);
void smk_cols_drop_layouts(ColsAux *aux);

hipError_t smk_bricks_dilate(const unsigned char *flags, const int nb[3], const int r[3], unsigned char *out, hipStream_t s);
// the flags of one table (version): buffers, and how many bricks came out flagged (copied back behind the kernel)
struct BrickSet {
  unsigned char *flags = nullptr;
  uint32_t *sat = nullptr;
  unsigned *d_count = nullptr, *h_count = nullptr;  // device word; pinned copy
  hipEvent_t counted = nullptr;
  size_t flags_cap = 0, sat_cap = 0;
  unsigned char *dil = nullptr;  // flags dilated by dil_r bricks per axis (perturbed fetch), made on demand
  size_t dil_cap = 0;
  int dil_r[3] = {-1, -1, -1};
  bool valid = false;
  float fill = -1.f;  // share of the bricks that are flagged; < 0: not known yet
};

// One cached time step (smk_timesteps.hip; DESIGN.md "Time steps"): what smk_upload_volume makes of a volume.  The buffers
// of a slot are reused by the step that replaces it (every step has the first upload's geometry).
struct TimeStep {
  int id = -1;                      // the host's time-step number; -1: slot empty
  long long written = 0;            // upload sequence number (the ring hands out the slot after the last one written)
  void *vox = nullptr;              // packed voxels of the stored box (region + halo)
  uint32_t *nrm = nullptr;          // separate packed normals (f32 with 4 channels and normals), else null
  float4 *mm = nullptr;             // brick min/max summaries (smk_bricks.hip)
  void *vox_x = nullptr;            // x-major copy, made on first use (smk_api.hip make_xmajor_copy)
  bool vox_x_valid = false;
  hipEvent_t ready = nullptr;       // end of an asynchronous upload, on the stream it was enqueued on
  bool ready_pending = false;       // ... recorded and not yet seen complete
  hipEvent_t used = nullptr;        // the last frame that read the step
  bool used_valid = false;
  hipEvent_t nonframe_read = nullptr;  // the last reader of the step that is no frame (a producer's source, the histogram, the read-back)
  bool nonframe_read_valid = false;
  int *pass1_words = nullptr;       // eight ints the first pass of a producer INTO this slot reduces into (a derive's six extremes, a merge's maximum)
  // what of the stored box holds the step's real voxels (DESIGN.md 3b "Stencil producers on a shard"): an upload fills the
  // stored box, a sharded stencil producer leaves a rim of zeros at every face that is no face of the volume
  int valid_halo = 1;               // halo voxels round the region that are exact: `halo` after an upload
  int vlo[3] = {0, 0, 0}, vhi[3] = {0, 0, 0};  // the valid box [vlo, vhi), global voxels
};

// One frame on its way to the host (smk_present.hip; DESIGN.md "Present"): everything a frame in flight needs that the
// context would otherwise share -- its RGBA8 and window-depth device buffers, their pinned host copies, its staged copy of
// the host's scene depth, its events.  Two of them, used in turn by the tickets of smk_render_present_begin.
struct PresentSlot {
  unsigned char *d_rgba8 = nullptr, *h_rgba8 = nullptr;  // [npix][4] bytes: device; pinned
  float *d_zwin = nullptr, *h_zwin = nullptr;            // [npix] window depths: device; pinned
  size_t cap = 0;                                        // pixels those four hold
  float *d_zscene = nullptr;                             // the host's scene depth, copied at `begin`
  size_t zscene_cap = 0;
  hipEvent_t pev0 = nullptr, pev1 = nullptr;             // around the present kernel (smk_get_stat "present_ms")
  hipEvent_t presented = nullptr, copied = nullptr;      // render stream: buffers written; copy stream: they are in host memory
  hipEvent_t ev0 = nullptr, ev1 = nullptr;               // the frame's pair of the timing ring (not owned)
  long long ticket = 0, frame_id = 0;
  bool outstanding = false;                              // begun and not ended
  bool want_depth = false, has_bg = false, has_scene = false;
  float bg[3] = {0, 0, 0};
  int zkind = 0;
  size_t npix = 0;                                       // the window the frame was begun with
};

struct smk_ctx {
  int device = 0;
  std::string err;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // ring of HIP-event pairs bracketing the render kernel of the last SMK_TIMING_RING frames,
  // recorded on the stream the kernel is launched on (bench.py's roofline leg reads them)
  std::vector<hipEvent_t> tev0, tev1;
  long long tcount = 0;

  // volume
  bool have_volume = false;
  int dtype = 0, nelts = 0, dmode = 0;
  int N[3] = {0, 0, 0};
  float fsize[3] = {1, 1, 1};
  int g0[3] = {0, 0, 0}, g1[3] = {0, 0, 0};  // this context's region
  int O[3] = {0, 0, 0}, D[3] = {0, 0, 0};
  int halo = 1;
  int region_on = 0;  // sub-box of renderVolume(.., xext, yext, zext): volume space
  float region_lo[3] = {0, 0, 0}, region_hi[3] = {0, 0, 0};
  int clip_axis = 0;  // orthogonal clip plane: 0 off, 1..6 = X+ X- Y+ Y- Z+ Z-
  float clip_vpos[3] = {0, 0, 0};
  int cplane_on = 0;  // free clip plane (glClipPlane), eye space
  double cplane_eye[4] = {0, 0, 0, 0};
  // the clip-plane widget's data slice (smk_set_clip_slice; smk_clip_slice.hip)
  int clip_slice_on = 0, clip_slice_look = 0;
  float clip_slice_corners[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  float clip_slice_alpha = 0, clip_slice_dv = 0;
  int clip_slice_pass = 0;  // the pass the last frame's rule chose: 0 none, 1 before, 2 after (smk_get_stat "clip_slice_pass")
  void *d_vox = nullptr;
  void *d_vox_x = nullptr;  // x-major copy [x][z][y] for views whose principal axis is x (lazy)
  float4 *d_brick_mm = nullptr;  // per brick of the stored box: range of the first two channels (smk_bricks.hip)
  int nbr[3] = {0, 0, 0};
  BrickSet br3;                        // brick flags under the dense 3-D table (the 2-D table's live in its versions)
  bool bricks3_dirty = true;
  std::string slab_why;     // why the last frame fell back to the gather kernel ("" if it did not)
  uint32_t *d_nrm = nullptr;
  bool have_normals = false;
  size_t vox_bytes = 0;
  // time steps: ts[ts_cur] is the step frames render (d_vox, d_nrm, d_brick_mm, d_vox_x point into it).  A context that
  // never calls the time-step entries holds its volume in ts[0] and records no events (ts_series false)
  std::vector<TimeStep> ts;
  int ts_cap = 1, ts_cur = -1, ts_cur_id = 0;
  long long ts_written = 0;
  bool ts_series = false;
  long long tblend_count = 0;  // blends enqueued by smk_blend_timesteps so far (smk_get_stat "tblend_count")

  // sharding
  int rank = 0, nranks = 1;

  // classification
  int tf_mode = -1;  // 0 1-D, 1 2-D, 2 3-D
  float4 *d_tlut = nullptr;
  int tlut_size = 0;
  std::vector<unsigned char> h_tf_vg, h_tf_h;
  unsigned char *d_tf_raw = nullptr;  // the table as it was set (the effective one = a 256-entry alpha map applied by a kernel)
  size_t tf_raw_cap = 0;
  bool tf_raw_stale = true, tf_raw_ev_valid = false;
  hipEvent_t tf_raw_ev = nullptr;     // the last kernel that read d_tf_raw
  hipStream_t tf_stream = nullptr;    // the table refresh runs here, beside the previous frame's ray-march
  hipEvent_t tf_ready = nullptr;      // ... and a frame's stream waits for this
  bool tf_ready_pending = false;
  uint32_t *d_tf_vg = nullptr, *d_tf_h = nullptr, *d_tf3d = nullptr;
  uint32_t *d_tf3d_occ = nullptr;  // occupancy of the dense 3-D table folded over its third axis (smk_set_tf3d)
  int tf3d_occ_roww = 0;
  uint32_t *d_tf_occ = nullptr;  // occupancy bitmap of the effective (V,G) table, tf_occ_roww words per row
  int tf_occ_roww = 0;
  // versions of the effective table + bitmap (d_tf_vg / d_tf_occ point into the current one): rebuilt without
  // stalling the frames in flight when the correction rate moves with the camera (smk_api.hip refresh_tf2d)
  struct TfVersion {
    unsigned char *d = nullptr, *h = nullptr;  // device copy; pinned staging
    BrickSet br;                                // this version's brick flags (smk_bricks.hip)
    size_t cap = 0;
    hipEvent_t copied = nullptr, used = nullptr;
    bool used_valid = false;
  } tfv[4];
  int tf_cur = -1;
  int sv = 0, sg = 0, s3v = 0, s3g = 0, s3h = 0;
  bool tf_dirty = true;
  float tf_rate_applied = -1.f;
  unsigned char tf_map_applied[256] = {0};  // the alpha-byte map the current effective table was made with
  bool tf_map_valid = false;

  // camera
  bool have_camera = false;
  double mv[16];
  float frustum[4], clip[2];
  int W = 0, H = 0;

  // sampling
  float sample_rate = 2.5f, gamma = 1.f;
  int steps = 0, scale_alphas = 1;

  // shading
  int blend = 0;  // smk_blend
  int shade = 0;
  float light_pos[3] = {0, 0, -5}, eye[3] = {0, 0, -7}, at[3] = {0, 0, 0};
  float xform[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float intens = .75f, amb = .05f;

  // half-angle-slicing shadows (smk_set_shadow)
  int shadow_on = 0, shadow_px = 1024;
  float shadow_q = .5f;
  float4 *d_light[2] = {nullptr, nullptr};  // ping-pong light buffers, light_cap texels each
  size_t light_cap = 0;
  int light_lb = 0;                         // the light buffer's edge in the last frame with shadows
  float4 *d_light_hist = nullptr;           // [nslices + 1][LB][LB]: every slice's light buffer (the two marches, smk_shadow.hip)
  size_t light_hist_cap = 0;                // texels
  const float4 *d_light_last = nullptr;     // the light buffer the last frame with shadows left (in d_light[] or the history)
  int opt_shadow_march = 1;                 // option "shadow_march": 1 = two marches (default), 0 = a launch per slice
  int opt_shadow_look = 0;                  // option "shadow_look": 0 the R8k look, 1 the NV20 look of NV20VolRen3D2 (smk.h smk_set_shadow)
  int opt_shadow_perturb = 0;               // option "shadow_perturb": 1 = a perturbed frame with shadows renders (0: refused, smk.h)
  unsigned *d_shadow_barrier = nullptr;     // the fused shadow launch's grid-barrier counter
  int light_hist_n = 0;                     // buffers the last march kept (nslices + 1; 0: none)
  long long light_hist_stride = 0;          // texels between two of them
  // shadows on a shard (smk_shadow_entries_device): X_{r->this} of every rank r, for the next frame
  float4 *d_shadow_entries = nullptr;
  size_t shadow_entries_cap = 0;            // texels
  bool shadow_entries_fresh = false;        // set since the last frame with shadows
  smk_shadowcoef shadow_entries_sc;         // the slice set they were made for
  float4 *d_shadow_exports = nullptr;       // phase 1's output of smk_shadow_exchange_local
  size_t shadow_exports_cap = 0;            // texels
  // halo refill between devices (smk_step_halo_exchange_local): this rank's exports [0] and entries [1], staged
  void *d_halo_stage[2] = {nullptr, nullptr};
  size_t halo_stage_cap[2] = {0, 0};        // bytes

  // perturbation
  uint32_t *d_noise = nullptr;
  std::vector<unsigned char> h_noise;  // what d_noise holds (smk_set_perturb replaces the device copy only when the bytes change)
  int nn = 0;
  float pw[4] = {0, 0, 0, 0}, ps[4] = {0, 0, 0, 0};

  // scratch output for host-pointer renders
  float4 *d_out = nullptr;
  float *d_depth = nullptr;
  size_t out_cap = 0;
  // smk_render_occluded: the host's scene depth staged for the frame (and its re-render)
  float *d_zscene = nullptr;
  size_t zscene_cap = 0;

  // frames handed to the host as RGBA8 + window depth (smk_present.hip)
  PresentSlot present[2];
  long long present_ticket = 0;            // the last ticket handed out (ticket t lives in slot t & 1)
  hipStream_t present_stream = nullptr;    // the device-to-host copies, beside the next frame's ray-march
  hipEvent_t present_ev[2] = {nullptr, nullptr};  // around the kernel of the last smk_present_device
  bool present_pending = false;            // ... recorded and not read yet
  float present_ms = 0;                    // smk_get_stat "present_ms"
  double present_bytes = 0;                // smk_get_stat "present_bytes"

  // options / stats
  int opt_kernel = 0, opt_tf_raw = 0;
  int opt_bricks = 1;      // brick flags on (0: every slice is streamed and sampled, as before round 2's last step)
  int opt_inject_status = 0;  // (test hook) the next slice-ring frame reports this status word
  int opt_wave_w = 8, opt_blk_w = 2, opt_lockstep = 1;
  SlabAux slab;  // slice-ring kernel side buffers
  ColsAux cols;  // column-stream kernel side buffers and knobs
  // auto mode (option kernel = 0) picks the ray-marcher by measurement: the first frames of a
  // new configuration run the slice-ring kernel, then the gather kernel (bit-identical frames),
  // and the faster one is kept for that configuration
  long long frame_id = 0;                  // frames enqueued so far (smk_last_frame_id)
  long long slab_failures = 0, slab_retries = 0;  // slice-ring frames flagged invalid / re-rendered by smk_render
  long long slab_lost = 0;  // ... of which flagged too late for anybody to be told (their status slot had been handed on)
  struct TuneEntry { int kernel; long long expires; };  // (a measured or forced choice is re-examined after a while)
  std::map<unsigned long long, TuneEntry> tune_choice;
  unsigned long long last_slab_sig = 0;  // configuration of the latest slice-ring launch (a failed one is not tried again)
  unsigned long long tune_sig = 0;
  int tune_state = 0, tune_slot[2] = {0, 0};
  long long tune_tcount = 0;  // frame count when the second timed trial was enqueued
  int last_kernel = 0;
  float last_ms = 0;
  double last_alg_bytes = 0;
};

// brick flags (smk_bricks.hip)
hipError_t smk_bricks_minmax(const void *vox, int dtype, const int D[3], const int nb[3], float4 *mm, hipStream_t s);
hipError_t smk_bricks_flags(const float4 *mm, const int nb[3], const uint32_t *occ, int roww, int sv, int sg, uint32_t *sat,
                            unsigned char *flags, unsigned *count, hipStream_t s);

// launchers (one translation unit per kernel family)
hipError_t smk_launch_gather(const RenderParams &P, int dtype, int tf_mode, int shade_kind,
                             hipStream_t s);
hipError_t smk_launch_count_inside(const RenderParams &P, unsigned long long *d_count, hipStream_t s);
// one launch per slice (smk_shadow.hip); L0 cleared by the caller
hipError_t smk_launch_shadow(const RenderParams &P, const smk_shadowcoef &sc, int dtype, int tf_mode, int shade_kind,
                             float4 *L0, float4 *L1, unsigned *barrier /* one device word for the fused launch's grid barrier, or null */, hipStream_t s);
hipError_t smk_launch_shadow_march(const RenderParams &P, const smk_shadowcoef &sc, int dtype, int tf_mode, float4 *hist, long long hstride,
                                   hipStream_t s);
// shadows on a shard: phase 1 (S.exports) and phase 2 (the march from the composed entries, into hist); the light samples
// of the box [olo, ohi] (smk_get_stat "light_samples")
hipError_t smk_launch_shadow_exports(const RenderParams &P, const smk_shadowcoef &sc, int dtype, int tf_mode, const SmkShadowShard &S,
                                     hipStream_t s);
hipError_t smk_launch_shadow_march_shard(const RenderParams &P, const smk_shadowcoef &sc, int dtype, int tf_mode, float4 *hist,
                                         long long hstride, const SmkShadowShard &S, hipStream_t s);
hipError_t smk_launch_shadow_count_light(const RenderParams &P, const smk_shadowcoef &sc, const float olo[3], const float ohi[3],
                                         unsigned long long *d_count, hipStream_t s);
// (smk_shadow_plan.hip) the frame with shadows a shard context would render now: its slice set and phase-1 parameters; the buffer
// for X_{r->this} (LB x LB texels per rank), made current for the next frame by smk_shadow_entries_commit
int smk_shadow_shard_setup(smk_ctx *c, RenderParams &P, smk_shadowcoef &sc, SmkShadowShard &S, hipStream_t s);
float4 *smk_shadow_entries_reserve(smk_ctx *c, int LB);
void smk_shadow_entries_commit(smk_ctx *c, const smk_shadowcoef &sc);
// plan + launch (smk_slab_plan.hip); returns hipErrorNotSupported (and *why) when the frame must use the gather kernel
hipError_t smk_launch_slab(RenderParams P, int dtype, int tf_mode, int shade_kind, const void *vox_native, const void *vox_xmajor, SlabAux *aux,
                           const char **why, hipStream_t s);
// the measured weights and depth cuts belong to the volume they were measured on: forgotten on a time-step switch
void smk_slab_forget_measurements(SlabAux *aux);
// the column-stream kernel (smk_cols_plan.hip); same convention as smk_launch_slab
hipError_t smk_launch_cols(RenderParams P, int dtype, int tf_mode, int shade_kind, const void *vox_native, ColsAux *aux, int *status_word,
                           const char **why, hipStream_t s);

// a few host threads for the per-frame planning (smk_api.hip): run(n, f) calls f(0) .. f(n - 1), f(0) on the caller
#include <functional>
int smk_host_pool_size();
void smk_host_pool_run(int n, const std::function<void(int)> &f);

// the geometry of a volume upload (smk_api.hip): every time step of a series has the first one's
struct SmkVolGeom {
  int dtype = 0, nelts = 0, dmode = 0;
  int N[3] = {0, 0, 0};
  float fs[3] = {0, 0, 0};
  int g0[3] = {0, 0, 0}, g1[3] = {0, 0, 0}, O[3] = {0, 0, 0}, D[3] = {0, 0, 0}, nbr[3] = {0, 0, 0};
  bool grad = false, padded = false;
  size_t vox_bytes = 0, nrm_bytes = 0, mm_bytes = 0;
};
int smk_volume_geometry(smk_ctx *c, const char *who, const smk_volume_desc *b, int nb, int nelts, smk_dtype dtype,
                        smk_datamode dmode, SmkVolGeom &g);
void smk_set_geometry(smk_ctx *c, const SmkVolGeom &g);
int smk_alloc_step(smk_ctx *c, const SmkVolGeom &g, TimeStep &T);
int smk_pack_step(smk_ctx *c, const char *who, const SmkVolGeom &g, const smk_volume_desc *b, int nb, bool on_device, TimeStep &T,
                  hipStream_t s);
// ts[k] becomes the step frames render (its brick flags are made again before the next frame)
void smk_use_step(smk_ctx *c, int k);

// n words a kernel of the latest frame wrote (ticks, counters), read once the device has finished it; synchronises
template <class T>
static int read_back(smk_ctx *c, T *h, const T *d, size_t n) {
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
  return 0;
}

// host set-up shared by the C ABI's files (smk_api.hip; hidden: not part of the library's interface)
#pragma GCC visibility push(hidden)
int smk_build_params(smk_ctx *c, RenderParams &P, hipStream_t s);  // a frame's RenderParams from the context (no shadows)
int smk_shade_kind(const smk_ctx *c);  // 0 none, 1 R8k, 2 NV20
void smk_region_box(const smk_ctx *c, const int g0[3], const int g1[3], float lo[3], float hi[3], int top[3]);
void smk_shard_region(const smk_ctx *c, int rank, int g0[3], int g1[3]);
// the region of shard `rank` of this context's series and the box of D voxels from O that rank stores, pad included
// (smk_volume_geometry's rule, from the series' dims and dtype and this context's option "halo")
void smk_shard_stored_box(const smk_ctx *c, int rank, int g0[3], int g1[3], int O[3], int D[3]);
void smk_bsp_order(const smk_ctx *c, const double pos[3], int *order);
void smk_inverse_affine(double inv[16], const double m[16]);
int smk_make_xmajor_copy(smk_ctx *c);
int smk_frame_buffers(smk_ctx *c);  // (smk_frame.hip)
// (smk_frame.hip) a frame enqueued on `stream` -- what smk_render[_occluded]_device do, d_zscene a DEVICE buffer or null --, and the
// status word of frame `id`, consumed: non-zero (with the reason in c->err) when a streaming kernel flagged the frame
int smk_frame_enqueue(smk_ctx *c, const char *who, void *d_rgba, void *d_depth, const float *d_zscene, int zkind, void *stream);
int smk_frame_check_status(smk_ctx *c, long long id);
// (smk_present.hip) frames begun and not ended; smk_get_stat "present_ms"; everything the slots own (smk_destroy)
bool smk_present_outstanding(const smk_ctx *c);
int smk_present_ms(smk_ctx *c, double *value);
void smk_present_free(smk_ctx *c);
void smk_slab_free(SlabAux *aux);  // (smk_slab_plan.hip)
// a ray's coefficients on the host, for planning, at a real-valued position (px, py) of the image plane (smk_slab_plan.hip)
void host_ray_at(const RenderParams &P, double px, double py, double A[3], double B[3]);
int smk_cols_stat(smk_ctx *c, const char *name, double *value);  // smk_get_stat "cols_*" (smk_cols_plan.hip)
int smk_slab_plan_stat(smk_ctx *c, const char *name, double *value);  // smk_get_stat "slab_plan_*" (smk_slab_plan.hip)
// frames with shadows (smk_shadow_plan.hip): the half-angle slices and boxes of P (S, halo_need: a shard's); the light
// samples a context owns (smk_get_stat); and a frame's shadow stage -- the light march (*marched), else the whole frame
// as a launch per slice
int smk_shadow_setup(smk_ctx *c, RenderParams &P, smk_shadowcoef &sc, SmkShadowShard *S, int *halo_need);
int smk_shadow_light_owned(smk_ctx *c, RenderParams &P, smk_shadowcoef &sc, float olo[3], float ohi[3]);
int smk_shadow_frame(smk_ctx *c, RenderParams &P, void *d_rgba, void *d_depth, hipStream_t s, bool *marched);
bool smk_shadow_light_along_view(const smk_ctx *c);  // the reference's axis[3] = vdl > 0 (compute_shadowcoef's front_to_back)
// the clip-plane widget's data slice composed onto the finished volume frame of P, on the frame's stream (smk_clip_slice.hip);
// launches nothing unless smk_set_clip_slice and the orthogonal clip plane are on
int smk_clip_slice_stage(smk_ctx *c, const RenderParams &P, hipStream_t s);
#pragma GCC visibility pop

// time steps (smk_timesteps.hip).  The step frames render is current; a frame's stream waits for its upload, and its end is
// recorded as the step's last reader (an upload that overwrites the slot waits for that)
int smk_step_wait_ready(smk_ctx *c, hipStream_t s);
int smk_step_mark_used(smk_ctx *c, hipStream_t s);
void smk_free_steps(smk_ctx *c);
// the slot that holds time step `timestep` (an id, or SMK_STEP_CURRENT), or -1
int smk_step_slot(const smk_ctx *c, int timestep);
// the slot of `timestep` for entry `who`, with the refusals that the histogram, the probe and the read-back of a step share
__attribute__((visibility("hidden"))) int step_slot(smk_ctx *c, const char *who, int timestep, int *k);
// a step of this context keeps its normals in a buffer of their own, TimeStep::nrm (smk_packed.h: four-channel f32)
inline bool smk_step_separate_normals(const smk_ctx *c) { return c->dtype == SMK_F32 && c->nelts == 4 && c->have_normals; }
// the bytes of that buffer: a word per voxel of the stored box, or 0
inline size_t smk_step_nrm_bytes(const smk_ctx *c) { return smk_step_separate_normals(c) ? (size_t)c->D[0] * c->D[1] * c->D[2] * 4 : 0; }
// the rows of this context's region in its stored box (smk_packed.h)
inline StepRows smk_step_rows(const smk_ctx *c) { return step_rows(c->g0, c->g1, c->O, c->D, c->dtype == SMK_F32); }
// Kernels on stream s that read or make resident steps and are no frame's: one bracket for all (smk_timesteps.hip, "Ordering").
// _read_begin: s is ordered behind the writer of slot k and behind its last reader that is no frame.
// _read: `launches` enqueues kernels that READ slots ka and kb (-1: none) behind their _read_begin; whatever it returns, the
//   slots' read events are then recorded on s -- the one place where that is done --, so a slot's next writer waits for them.
// _produce: entry `who` makes step `id` from slots ka and kb (the sources; -1: none), as a _read of them.  The output takes a
//   cached id's own slot, else one by the ring's rule that is neither a source's nor the current step's: a ring of fewer slots
//   than 1 + the distinct slots among the sources and the current step refuses the call.  s is ordered behind the output slot's
//   old readers and writers, the slot is emptied and its buffers are made; `launches(out, a, b)` enqueues the kernels that fill
//   `out` from the sources' slots (null: none); then the brick summaries are made, the slot holds step `id`, its `ready` event
//   is recorded on s and a current step overwritten in place is switched to.  After a failed launch the slot stays empty.
int smk_step_read_begin(smk_ctx *c, int k, hipStream_t s);
#pragma GCC visibility push(hidden)
int smk_step_read(smk_ctx *c, int ka, int kb, hipStream_t s, const std::function<int()> &launches);
using StepLaunches = std::function<int(TimeStep &out, const TimeStep *a, const TimeStep *b)>;
int smk_step_produce(smk_ctx *c, const char *who, int id, int ka, int kb, hipStream_t s, const StepLaunches &launches);
// _rewrite: `launches` enqueues kernels that WRITE voxels of the cached step in slot k in place (the halo refill,
//   smk_step_halo.hip).  s is ordered behind the slot's frames, readers and writer, as for any writer, but the slot keeps its
//   id and its place in the ring's order; then the brick summaries are made again for the stored voxels, the x-major copy is
//   dropped, the slot's `ready` event is recorded on s -- also after a failed launch: every later reader waits for whatever
//   was enqueued -- and a current step is switched to, as after an in-place upload.  `launches` sets what is valid of the step.
int smk_step_rewrite(smk_ctx *c, int k, hipStream_t s, const std::function<int(TimeStep &)> &launches);
// What the stencil producers (smk_step_derive.hip, smk_step_merge.hip, smk_step_merge_h.hip; what their host sides say alike:
// smk_step_stencil.h) refuse before they look at their data, in this order:
// no volume; a sharded context (sharded_why: the entry's reason); the series' nelts (nelts_why: the entry's refusal behind
// "who: ", empty when they suit); a stored box that is not what the kernels take for granted; a volume without an interior
// voxel (as prep_entry); then, with step_src (null: dense arrays), a source that is not cached (*ksrc: its slot), and the ids
struct StencilEntry {
  const char *who, *sharded_why;
  std::string nelts_why;
  const char *prep_entry;
};
int smk_step_stencil_refusals(smk_ctx *c, const StencilEntry &E, int step_out, const int *step_src, int *ksrc);
// The stencil producers' shard entries (smk_*_timestep_shard, smk_step_extremes_device): a stored box anywhere in the volume.
// _shard_refusals: no volume; the series' nelts; a stored box that is not what the shard kernels take for granted; a volume
// without an interior voxel; a source that is not cached (*ksrc: its slot); with step_out (null: the export, a reader) the ids;
// a source whose valid halo is below reach + 1.  SmkShardBox: what the kernels get of the geometry, in LOCAL voxels of the
// stored box -- the region, and with `out` the valid box of the result, which _shard_done then writes into the output slot
struct SmkShardBox {
  int O[3], r0[3], r1[3], v0[3], v1[3];
};
int smk_step_shard_refusals(smk_ctx *c, const StencilEntry &E, int reach, int step_src, const int *step_out, int *ksrc);
void smk_step_shard_box(const smk_ctx *c, const TimeStep &src, int reach, SmkShardBox &B);
void smk_step_shard_done(const smk_ctx *c, const TimeStep &src, int reach, const SmkShardBox &B, TimeStep &out);
// smk_step_extremes_device's two kinds: pass 1 of the shard instances over the region, into the caller's eight words
int smk_derive_extremes_enqueue(smk_ctx *c, const char *who, int step_src, int compat, void *d_words, hipStream_t s);  // (smk_step_derive.hip)
int smk_merge_extremes_enqueue(smk_ctx *c, const char *who, int step_src, void *d_words, hipStream_t s);               // (smk_step_merge.hip)
// The block entries (smk.h: smk_block; smk_step_block.hip, and the block instances of the three stencil producers): a rank's own
// dense block of the volume.  SmkBlockView: what the entries make of a block against this context's stored box -- C = block ∩
// stored box ∩ volume in GLOBAL voxels, the source's valid halo, and the pitches with their zeros resolved.
// smk_block_view: the refusals every block entry shares (a NULL block, sizes, pitches, a block outside the volume, a C that
//   does not contain the region) and the view.
// smk_step_block_refusals: a stencil form's, in the twins' order -- no volume; the series' nelts; the stored box; a volume
//   without an interior voxel; with step_out (null: the export) the id --, then smk_block_view's, then on a sharded context a
//   source valid halo below reach + 1.
// _block_box / _block_done: smk_step_shard_box / _done with C in the place of the source slot's valid box.
struct SmkBlockView {
  int c0[3], c1[3];
  int halo;
  long long py, pz;
};
int smk_block_view(smk_ctx *c, const char *who, const smk_block *b, SmkBlockView &V);
int smk_step_block_refusals(smk_ctx *c, const StencilEntry &E, int reach, const int *step_out, const smk_block *b, SmkBlockView &V);
void smk_step_block_box(const smk_ctx *c, const SmkBlockView &V, int reach, SmkShardBox &B);
void smk_step_block_done(const smk_ctx *c, const SmkBlockView &V, int reach, const SmkShardBox &B, TimeStep &out);
// smk_block_extremes_device's merge kind (smk_step_merge.hip); the derive kind lives beside the entry (smk_step_derive.hip)
int smk_merge_block_extremes_enqueue(smk_ctx *c, const char *who, const void *const *d_fields, int nf, smk_dtype dtype, const smk_block *b,
                                     void *d_words, hipStream_t s);
// The packed voxels of a whole stored box in one pass (smk_step_block.hip): inside the box [c0, c1) (LOCAL voxels of the stored
// box; empty: nowhere) the voxels of the block whose element [0][0][0] is local voxel bo, read through its pitches; elsewhere in
// the volume zeros with the normal (128, 128, 128); zeros in the pad column and row.  src null: zeros everywhere (smk_declare_volume)
hipError_t smk_pack_block(const smk_ctx *c, const void *src, const unsigned char *grad, const int bo[3], const int c0[3], const int c1[3],
                          long long py, long long pz, TimeStep &T, hipStream_t s);
// the valid halo of the step frames render, for the frame path's comparisons with a need
int smk_step_shown_halo(const smk_ctx *c);
#pragma GCC visibility pop
