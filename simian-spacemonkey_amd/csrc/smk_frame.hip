// smk_frame.hip -- a frame: the driver behind smk_render_device / smk_render as a sequence of stages (frame_open, the shadow
// stage of smk_shadow_plan.hip, the kernel choice, one launch per ray-marcher, the clip slice of smk_clip_slice.hip,
// frame_close), the auto mode's choice between the slice-ring and the gather kernel, the per-frame status words and the
// timing ring.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "smk_internal.h"

extern "C" int smk_timing_reset(smk_ctx *c) {
  if (!c) return 1;
  c->tcount = 0;
  return 0;
}

// average render-kernel duration over the frames recorded since smk_timing_reset (at most the
// last SMK_TIMING_RING); synchronises the device
extern "C" int smk_timing_read(smk_ctx *c, float *avg_ms, int *nframes) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  int n = (int)std::min<long long>(c->tcount, SMK_TIMING_RING);
  double sum = 0;
  for (int i = 0; i < n; ++i) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->tev0[i], c->tev1[i]));
    sum += ms;
  }
  if (avg_ms) *avg_ms = n ? (float)(sum / n) : 0.f;
  if (nframes) *nframes = n;
  return 0;
}

extern "C" int smk_last_frame_info(smk_ctx *c, int *kernel, float *ms, double *alg_bytes) {
  if (!c) return 1;
  if (kernel) *kernel = c->last_kernel;
  if (ms) *ms = c->last_ms;
  if (alg_bytes) *alg_bytes = c->last_alg_bytes;
  return 0;
}

// Slice-ring kernel error words -> failed frames (the kernel never hangs and never returns a frame
// built from unloaded data silently).  Every frame has its own word, SMK_STATUS_RING of them in turn.
// A caller that keeps frames in flight asks per frame (smk_frame_failed, after synchronising with it)
// and renders a flagged frame again; a flag nobody asked about fails the NEXT render call loudly.
// The status word of frame `id` (slot id % SMK_STATUS_RING), consumed: 0 = none.  Words carry the id of the frame that wrote
// them (a slice-ring frame may write late, into a slot that has since been handed to a younger frame): one of ANOTHER frame
// is counted as that frame's failure and left alone for whoever owns it -- or dropped when that frame is out of the ring.
static int take_status(smk_ctx *c, long long id) {
  if (!c->slab.h_status || id <= 0) return 0;
  volatile int *w = (volatile int *)c->slab.h_status + (int)(id % SMK_STATUS_RING);
  const int st = *w;
  if (!st) return 0;
  const long long tag = (st >> 8) & 0x7fffff;
  if (tag != (id & 0x7fffff)) {
    // a late word of an older frame of this slot: nobody can be told about that frame any more
    if (((id - tag) & 0x7fffff) % SMK_STATUS_RING == 0 && tag != 0) {
      *w = 0;
      ++c->slab_failures;
      ++c->slab_lost;
    }
    return 0;
  }
  *w = 0;
  ++c->slab_failures;
  // not again soon: in auto mode that configuration is the gather kernel's for a while
  if (c->opt_kernel == 0 && c->last_slab_sig) c->tune_choice[c->last_slab_sig] = {1, c->frame_id + 256};
  return st & 0xff;
}

static const char *status_text(int st) {
  return st == 1 ? "a streaming kernel reported a producer/consumer time-out" : st == 2 ? "the slice-ring kernel reported a window outside its host bound"
         : st == 3 ? "the column-stream kernel reported a job whose rays do not fit its lanes or its list" : "the column-stream kernel reported a ray it cannot list";
}

// frame `id` was flagged and nobody has asked about it: the call fails
static int check_frame_status(smk_ctx *c, long long id) {
  const int st = take_status(c, id);
  if (st) FAIL(c, "%s (status %d, frame %lld); frame invalid", status_text(st), st, id);
  return 0;
}

extern "C" long long smk_last_frame_id(smk_ctx *c) { return c ? c->frame_id : 0; }

extern "C" int smk_frame_failed(smk_ctx *c, long long frame_id) {
  if (!c) return 1;
  if (frame_id <= 0 || frame_id > c->frame_id || frame_id + SMK_STATUS_RING <= c->frame_id) return -1;  // never enqueued, or out of the ring: unknown
  return take_status(c, frame_id) ? 1 : 0;
}

// the status words (pinned, device-visible) and the diagnostic counters, made by the first frame of a streaming kernel
static int status_ring_ready(smk_ctx *c) {
  if (c->slab.h_status) return 0;
  HIPCHK(c, hipHostMalloc((void **)&c->slab.h_status, SMK_STATUS_RING * sizeof(int), hipHostMallocMapped));
  for (int k = 0; k < SMK_STATUS_RING; ++k) c->slab.h_status[k] = 0;
  HIPCHK(c, hipMalloc((void **)&c->slab.d_diag, SMK_SLAB_NDIAG * sizeof(float)));
  return 0;
}

// test hook (option inject_slab_status): what a failed frame leaves behind, once
static void inject_status(smk_ctx *c) {
  if (c->opt_inject_status && c->slab.h_status) {
    ((volatile int *)c->slab.h_status)[c->slab.status_slot] = c->slab.status_tag | c->opt_inject_status;
    c->opt_inject_status = 0;
  }
}

// ------------------------------------------------------------------------------- frame stages

// The frame's outputs, its algorithmic bytes, its event pair and its status word.
static int frame_open(smk_ctx *c, RenderParams &P, void *d_rgba, void *d_depth) {
  P.out = (float4 *)d_rgba;
  P.depth = (float *)d_depth;
  // algorithmic bytes: every stored voxel once + TF + RGBA f32 frame
  size_t nst = (size_t)c->D[0] * c->D[1] * c->D[2];
  double bv = c->dtype == SMK_U8 ? (double)c->nelts : c->dtype == SMK_U16 ? 2.0 * c->nelts : 4.0 * c->nelts;
  if (smk_shade_kind(c)) bv += 3.0;
  double tfb = c->tf_mode == 0 ? 16.0 * c->tlut_size
               : c->tf_mode == 1 ? 4.0 * c->sv * c->sg * (P.third_axis ? 2 : 1)
                                 : 4.0 * c->s3v * c->s3g * c->s3h;
  c->last_alg_bytes = (double)nst * bv + tfb + 16.0 * c->W * c->H;
  if (P.zscene) c->last_alg_bytes += 4.0 * c->W * c->H;  // (the host's scene depth: one float per pixel read)
  if (c->tev0.empty()) {
    c->tev0.resize(SMK_TIMING_RING);
    c->tev1.resize(SMK_TIMING_RING);
    for (int i = 0; i < SMK_TIMING_RING; ++i) {
      HIPCHK(c, hipEventCreate(&c->tev0[i]));
      HIPCHK(c, hipEventCreate(&c->tev1[i]));
    }
  }
  int slot = (int)(c->tcount % SMK_TIMING_RING);
  c->ev0 = c->tev0[slot];
  c->ev1 = c->tev1[slot];
  // (ev0 is recorded by the launcher right before the kernel: host-side planning between the two
  //  events would otherwise count as kernel time whenever the stream is idle)
  // kernel choice: the slice-ring kernel when it applies (2-D / separable classification,
  // no perturbation, rays sharing one principal axis), the generic gather kernel otherwise
  c->last_kernel = 1;
  c->slab_why.clear();
  // The status word this frame takes over belongs to frame id - SMK_STATUS_RING: flagged, and nobody has asked about it
  // (smk_frame_failed) while they could -- the call fails.  Younger frames' words are left for their owners: a host that
  // pipelines frames asks about frame i AFTER enqueuing frame i + 1 (sortlast.Pipeline), and must find the word there.
  if (check_frame_status(c, c->frame_id + 1 - SMK_STATUS_RING)) return 1;
  ++c->frame_id;
  c->slab.status_slot = (int)(c->frame_id % SMK_STATUS_RING);
  c->slab.status_tag = c->cols.status_tag = (int)((c->frame_id & 0x7fffff) << 8);
  if (c->slab.h_status) ((volatile int *)c->slab.h_status)[c->slab.status_slot] = 0;
  return 0;
}

struct KernelChoice {
  bool try_slab;
  unsigned long long sig;  // the configuration's signature (auto mode)
  int trial;               // 0 .. SMK_TUNE_SETTLE + 2: this frame is that trial frame of a new configuration; -1: none
};

// Auto mode: which kernel for this configuration?  A measured choice holds for a while; a new configuration gets trial frames.
static KernelChoice choose_kernel(smk_ctx *c, const RenderParams &P, bool with_depth, hipStream_t s) {
  KernelChoice k = {c->opt_kernel != 1 && c->opt_kernel != 3, 0, -1};
  if (c->opt_kernel != 0) return k;
  int as = 0;
  for (int a = 1; a < 3; ++a)
    if (fabsf(P.rc.Bc[a]) > fabsf(P.rc.Bc[as])) as = a;
  const unsigned long long f[] = {(unsigned long long)c->dtype, (unsigned long long)c->nelts, (unsigned long long)c->D[0],
                                  (unsigned long long)c->D[1], (unsigned long long)c->D[2], (unsigned long long)c->W,
                                  (unsigned long long)c->H, (unsigned long long)P.rc.nplanes, (unsigned long long)smk_shade_kind(c),
                                  (unsigned long long)P.third_axis, (unsigned long long)(as * 2 + (P.rc.Bc[as] > 0)),
                                  (unsigned long long)c->sv, (unsigned long long)c->sg, (unsigned long long)with_depth,
                                  (unsigned long long)P.pert_on, (unsigned long long)c->tf_mode, (unsigned long long)c->s3v,
                                  (unsigned long long)c->s3g, (unsigned long long)c->s3h, (unsigned long long)c->blend,
                                  (unsigned long long)P.sh.on, (unsigned long long)(P.zscene != nullptr)};
  k.sig = 1469598103934665603ull;
  for (unsigned long long v : f) k.sig = (k.sig ^ v) * 1099511628211ull;
  auto it = c->tune_choice.find(k.sig);
  if (it != c->tune_choice.end() && it->second.expires <= c->frame_id) {  // measured long ago: measure again
    c->tune_choice.erase(it);
    it = c->tune_choice.end();
    c->tune_sig = 0;
  }
  if (it != c->tune_choice.end()) {
    k.try_slab = it->second.kernel == 2;
    return k;
  }
  if (c->tune_sig != k.sig) {
    c->tune_sig = k.sig;
    c->tune_state = 0;
  }
  // Trial frames of a new configuration: SMK_TUNE_SETTLE untimed slice-ring frames -- its schedule and depth cuts come
  // from the workgroup times of earlier frames, so each waits for the one before it (a one-time stall; without it, and
  // with a single untimed frame, the timed trial was the first frame with cuts, 1.14 ms on a 1/8 shard that settles at
  // 0.15, and auto mode kept the 0.69 ms gather kernel for the shard) --, one untimed gather frame, then the timed pair.
  if (c->tune_state == SMK_TUNE_SETTLE + 3) {  // both timed trials issued: decide once their events have completed
    float ms_s = 0, ms_g = 0;
    // (a host that enqueues frames far ahead of the GPU would recycle the trials' event pairs -- the ring holds the
    //  last 64 frames -- before they complete, and the comparison would then be between two later frames of the
    //  same kernel: wait for the trials rather than let their slots go)
    if (c->tcount - c->tune_tcount >= SMK_TIMING_RING - 8) (void)hipEventSynchronize(c->tev1[c->tune_slot[1]]);
    if (hipEventQuery(c->tev1[c->tune_slot[0]]) == hipSuccess && hipEventQuery(c->tev1[c->tune_slot[1]]) == hipSuccess &&
        hipEventElapsedTime(&ms_s, c->tev0[c->tune_slot[0]], c->tev1[c->tune_slot[0]]) == hipSuccess &&
        hipEventElapsedTime(&ms_g, c->tev0[c->tune_slot[1]], c->tev1[c->tune_slot[1]]) == hipSuccess) {
      c->tune_choice[k.sig] = {ms_s <= ms_g ? 2 : 1, c->frame_id + 1024};
      k.try_slab = ms_s <= ms_g;
      if (getenv("SMK_DEBUG")) fprintf(stderr, "[smk] auto mode: slice-ring %.3f ms, gather %.3f ms (frame %lld)\n", ms_s, ms_g, c->frame_id);
    }  // else: keep the slice-ring kernel for this frame and ask again
    (void)hipGetLastError();
  } else {
    k.trial = c->tune_state;
    k.try_slab = k.trial != SMK_TUNE_SETTLE && k.trial != SMK_TUNE_SETTLE + 2;
    if (k.try_slab && k.trial > 0) (void)hipStreamSynchronize(s);  // (the previous settle frame's workgroup times are back)
  }
  return k;
}

// the column-stream kernel, forced (smk_cols_plan.hip)
static int launch_cols(smk_ctx *c, const RenderParams &P, hipStream_t s) {
  if (status_ring_ready(c)) return 1;
  const char *why = nullptr;
  c->cols.frame_ev0 = c->ev0;
  hipError_t e = smk_launch_cols(P, c->dtype, c->tf_mode, smk_shade_kind(c), c->d_vox, &c->cols,
                                 c->slab.h_status + c->slab.status_slot, &why, s);
  if (e == hipErrorNotSupported) {
    c->slab_why = why ? why : "?";
    FAIL(c, "smk_render: column-stream kernel forced but not applicable: %s", c->slab_why.c_str());
  }
  HIPCHK(c, e);
  c->last_kernel = 4;
  inject_status(c);
  return 0;
}

// the slice-ring kernel (smk_slab_plan.hip), made with the x-major copy where the view needs it; a frame it declines is the
// gather kernel's (and in auto mode no trial)
static int launch_slab(smk_ctx *c, const RenderParams &P, KernelChoice &k, bool ev0_recorded, hipStream_t s) {
  if (status_ring_ready(c)) return 1;
  if (c->opt_lockstep & 16) HIPCHK(c, hipMemsetAsync(c->slab.d_diag, 0, SMK_SLAB_NDIAG * sizeof(float), s));
  const char *why = nullptr;
  c->slab.frame_ev0 = ev0_recorded ? nullptr : c->ev0;
  hipError_t e = smk_launch_slab(P, c->dtype, c->tf_mode, smk_shade_kind(c), c->d_vox, c->d_vox_x, &c->slab, &why, s);
  if (e == hipErrorNotSupported && why && !strcmp(why, "x-major copy unavailable")) {
    if (smk_make_xmajor_copy(c)) return 1;
    e = smk_launch_slab(P, c->dtype, c->tf_mode, smk_shade_kind(c), c->d_vox, c->d_vox_x, &c->slab, &why, s);
  }
  if (e == hipSuccess) {
    c->last_kernel = 2;
    c->last_slab_sig = k.sig;
    inject_status(c);
  } else if (e == hipErrorNotSupported) {
    c->slab_why = why ? why : "?";
    if (c->opt_kernel == 2) FAIL(c, "smk_render: slab kernel forced but not applicable: %s", c->slab_why.c_str());
    // Not remembered: most reasons depend on the pose (too oblique, window does not fit LDS, ...)
    // and the signature does not; the next frame is planned afresh (planning runs per frame anyway)
    // and returns to the slice-ring kernel as soon as the view allows.
    if (c->opt_kernel == 0) k.trial = -1;
  } else
    HIPCHK(c, e);
  return 0;
}

// the gather kernel (smk_gather.hip): every frame no other kernel took
static int launch_gather(smk_ctx *c, const RenderParams &P, bool ev0_recorded, hipStream_t s) {
  if (!ev0_recorded) HIPCHK(c, hipEventRecord(c->ev0, s));
  HIPCHK(c, smk_launch_gather(P, c->dtype, c->tf_mode, smk_shade_kind(c), s));
  return 0;
}

// The end of the frame's kernel time; a trial's event pair is kept for the comparison; the table version and the time step
// the frame read are marked as in use until it completes.
static int frame_close(smk_ctx *c, hipStream_t s, int trial) {
  HIPCHK(c, hipEventRecord(c->ev1, s));
  if (trial >= 0) {
    if (trial >= SMK_TUNE_SETTLE + 1) {
      c->tune_slot[trial - (SMK_TUNE_SETTLE + 1)] = (int)(c->tcount % SMK_TIMING_RING);  // (this frame's event pair)
      c->tune_tcount = c->tcount;
    }
    c->tune_state = trial + 1;
  }
  if (c->tf_mode == 1 && c->tf_cur >= 0) {  // this frame read the current table version (refresh_tf2d waits for this before rewriting it)
    HIPCHK(c, hipEventRecord(c->tfv[c->tf_cur].used, s));
    c->tfv[c->tf_cur].used_valid = true;
  }
  if (smk_step_mark_used(c, s)) return 1;  // (and the time step it rendered)
  c->tcount++;
  return 0;
}

// The kind of a scene depth handed to smk_render_occluded[_device] (checked with or without a buffer)
static int scene_depth_kind_check(smk_ctx *c, const char *who, int kind) {
  if (kind != SMK_SCENE_VIEW_DEPTH && kind != SMK_SCENE_WINDOW_DEPTH)
    FAIL(c, "%s: bad scene depth kind %d (SMK_SCENE_VIEW_DEPTH = 0 or SMK_SCENE_WINDOW_DEPTH = 1)", who, kind);
  return 0;
}

// A frame on `stream`; d_zscene: the host's opaque scene depth on the device ([H][W] floats of that kind), or null
static int render_frame(smk_ctx *c, const char *who, void *d_rgba, void *d_depth, const float *d_zscene, int zkind, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!d_rgba) FAIL(c, "%s: null output", who);
  RenderParams P;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (smk_build_params(c, P, s)) return 1;
  if (d_zscene) {
    P.zscene = d_zscene;
    P.zscene_kind = zkind;
    const double n = c->clip[0], f = c->clip[1];
    if (zkind == SMK_SCENE_WINDOW_DEPTH && !(f > n))
      FAIL(c, "%s: window depths need a far plane beyond the near plane (clip = %g, %g)", who, n, f);
    P.zs_fn = f * n;
    P.zs_f = f;
    P.zs_fmn = f - n;
  }
  if (frame_open(c, P, d_rgba, d_depth)) return 1;
  bool marched = false;  // (a frame with shadows opens the kernel-time bracket before its light march)
  if (c->shadow_on) {
    if (smk_shadow_frame(c, P, d_rgba, d_depth, s, &marched)) return 1;
    if (!marched) return smk_clip_slice_stage(c, P, s) ? 1 : frame_close(c, s, -1);  // (a launch per slice: the whole frame)
  }
  KernelChoice k = choose_kernel(c, P, d_depth != nullptr, s);
  if (c->opt_kernel == 3 && launch_cols(c, P, s)) return 1;
  if (k.try_slab) {
    if (launch_slab(c, P, k, marched, s)) return 1;
  } else if (c->opt_kernel == 2)
    FAIL(c, "smk_render: slab kernel forced but classification mode %d is gather-only", c->tf_mode);
  if (c->last_kernel == 1 && launch_gather(c, P, marched, s)) return 1;
  // the clip-plane widget's data slice (smk_clip_slice.hip) composes onto the finished volume frame, whichever ray-marcher
  // made it, before the frame's completion event (and so before a shard's exchange); nothing is launched unless it is on
  if (smk_clip_slice_stage(c, P, s)) return 1;
  return frame_close(c, s, k.trial);
}

extern "C" int smk_render_device(smk_ctx *c, void *d_rgba, void *d_depth, void *stream) {
  return render_frame(c, "smk_render_device", d_rgba, d_depth, nullptr, 0, stream);
}

extern "C" int smk_render_occluded_device(smk_ctx *c, const void *d_scene_depth, int kind, void *d_rgba, void *d_depth, void *stream) {
  if (!c) return 1;
  if (scene_depth_kind_check(c, "smk_render_occluded_device", kind)) return 1;
  return render_frame(c, "smk_render_occluded_device", d_rgba, d_depth, (const float *)d_scene_depth, kind, stream);
}

int smk_frame_enqueue(smk_ctx *c, const char *who, void *d_rgba, void *d_depth, const float *d_zscene, int zkind, void *stream) {
  return render_frame(c, who, d_rgba, d_depth, d_zscene, zkind, stream);
}

int smk_frame_check_status(smk_ctx *c, long long id) { return check_frame_status(c, id); }

// the context's own W x H frame and depth buffers (smk_render, smk_render_slice)
int smk_frame_buffers(smk_ctx *c) {
  const size_t npix = (size_t)c->W * c->H;
  if (npix > c->out_cap) {
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->d_depth) (void)hipFree(c->d_depth);
    c->d_out = nullptr;
    c->d_depth = nullptr;
    HIPCHK(c, hipMalloc((void **)&c->d_out, npix * 16));
    HIPCHK(c, hipMalloc((void **)&c->d_depth, npix * 4));
    c->out_cap = npix;
  }
  return 0;
}

// A frame to host memory, rendered again on the gather kernel if the slice-ring kernel flags it; scene_depth: the host's
// opaque scene depth in HOST memory, or null
static int render_host(smk_ctx *c, const char *who, float *rgba, float *depth, const float *scene_depth, int zkind) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!rgba) FAIL(c, "%s: null output", who);
  if (!c->have_camera) FAIL(c, "%s: no camera set", who);
  size_t npix = (size_t)c->W * c->H;
  if (smk_frame_buffers(c)) return 1;
  const float *d_zscene = nullptr;
  if (scene_depth) {  // (staged in the context's buffer: the re-render below reads the same one)
    if (npix > c->zscene_cap) {
      if (c->d_zscene) (void)hipFree(c->d_zscene);
      c->d_zscene = nullptr;
      c->zscene_cap = 0;
      HIPCHK(c, hipMalloc((void **)&c->d_zscene, npix * 4));
      c->zscene_cap = npix;
    }
    HIPCHK(c, hipMemcpy(c->d_zscene, scene_depth, npix * 4, hipMemcpyHostToDevice));
    d_zscene = c->d_zscene;
  }
  if (render_frame(c, who, c->d_out, depth ? c->d_depth : nullptr, d_zscene, zkind, c->stream)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1));
  if (check_frame_status(c, c->frame_id)) {
    // the synchronous entry still owes its caller this frame: in auto mode it is rendered again, by
    // the gather kernel (take_status has just retired the slice-ring kernel for this configuration)
    if (c->opt_kernel != 0) return 1;
    const std::string first = c->err;
    ++c->slab_retries;
    if (render_frame(c, who, c->d_out, depth ? c->d_depth : nullptr, d_zscene, zkind, c->stream)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->last_kernel != 1 || check_frame_status(c, c->frame_id)) {
      c->err = first;
      return 1;
    }
    fprintf(stderr, "[smk] %s -- frame rendered again by the gather kernel\n", first.c_str());
  }
  HIPCHK(c, hipMemcpy(rgba, c->d_out, npix * 16, hipMemcpyDeviceToHost));
  if (depth) HIPCHK(c, hipMemcpy(depth, c->d_depth, npix * 4, hipMemcpyDeviceToHost));
  return 0;
}

extern "C" int smk_render(smk_ctx *c, float *rgba, float *depth) { return render_host(c, "smk_render", rgba, depth, nullptr, 0); }

extern "C" int smk_render_occluded(smk_ctx *c, const float *scene_depth, int kind, float *rgba, float *depth) {
  if (!c) return 1;
  if (scene_depth_kind_check(c, "smk_render_occluded", kind)) return 1;
  return render_host(c, "smk_render_occluded", rgba, depth, scene_depth, kind);
}
