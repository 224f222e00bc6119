// smk_present.hip -- the hand-over to the host: a finished float frame becomes what an 8-bit GL framebuffer takes (RGBA8,
// optionally composed over an opaque background colour, and the float32 window depth of the first-hit view depth), in
// pinned host memory, the copy of frame k running beside the ray-march of frame k + 1 (DESIGN.md "Present").
//   smk_present_device                      the conversion alone, on the caller's stream
//   smk_render_present                      render, present, copy; synchronous
//   smk_render_present_begin / _end         the same frame in two calls, two frames in flight
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "smk_internal.h"

// ------------------------------------------------------------------------------- the rule (tests/_present_ref.py restates it)

// q(x) = floor(sat(x) * 255 + 0.5); NaN -> 0.  One rounded fp32 operation per line (the library is built with
// -ffp-contract=off: the product and the sum stay two roundings).
__device__ __forceinline__ uint32_t present_q(float x) {
  x = x > 0.0f ? x : 0.0f;  // (NaN and -0.0 fail the comparison)
  x = x < 1.0f ? x : 1.0f;
  const float s = x * 255.0f;
  const float r = s + 0.5f;
  return (uint32_t)floorf(r);
}

// premultiplied (C, A) -> packed RGBA8, R in byte 0.  No background: every channel through q.  Background b: the reference's
// quad drawn UNDER the frame with GL_ONE_MINUS_DST_ALPHA, GL_ONE (gluvv.cpp:606-623), rgb = q(C + (1 - A) b), a = 255.
template <bool BG>
__device__ __forceinline__ uint32_t present_pixel(float4 v, float b0, float b1, float b2) {
  if (!BG) return present_q(v.x) | (present_q(v.y) << 8) | (present_q(v.z) << 16) | (present_q(v.w) << 24);
  const float t = 1.0f - v.w;
  const float u0 = t * b0, u1 = t * b1, u2 = t * b2;
  const float c0 = v.x + u0, c1 = v.y + u1, c2 = v.z + u2;
  return present_q(c0) | (present_q(c1) << 8) | (present_q(c2) << 16) | 0xff000000u;
}

// view depth d -> window depth z_w = f (d - n) / ((f - n) d) in [0, 1] (the inverse of smk_render_occluded's
// SMK_SCENE_WINDOW_DEPTH conversion), in double, rounded to float once.  Nothing hit (+inf) and NaN: exactly 1; d <= n: 0.
__device__ __forceinline__ float present_zw(float df, double n, double f, double fmn) {
  const double d = (double)df;
  if (!(d < (double)INFINITY)) return 1.0f;  // +inf, NaN
  if (d <= n) return 0.0f;
  const double num = f * (d - n);
  const double den = fmn * d;
  double zw = num / den;
  zw = zw < 0.0 ? 0.0 : zw;
  zw = zw > 1.0 ? 1.0 : zw;
  return (float)zw;
}

// A thread takes four consecutive pixels: four 16-B loads, ONE 16-B store of the packed bytes (a wave writes 1 KiB
// contiguously), and for depth one 16-B load and one 16-B store.  VEC8 / VECZ: the byte output / both depth planes are
// 16-B aligned; otherwise, and for the last npix % 4 pixels, a pixel at a time (4-B stores).  No LDS; grid-stride.
template <bool BG, bool VEC8, bool VECZ>
__global__ void __launch_bounds__(256) smk_k_present(const float4 *__restrict__ in, const float *__restrict__ depth, uint32_t *__restrict__ out8,
                                                     float *__restrict__ zwin, long long npix, float b0, float b1, float b2, double n,
                                                     double f, double fmn) {
  const long long ngroups = (npix + 3) >> 2;
  for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (long long)gridDim.x * blockDim.x) {
    const long long p0 = g << 2;
    if (p0 + 4 <= npix) {
      const float4 v0 = in[p0], v1 = in[p0 + 1], v2 = in[p0 + 2], v3 = in[p0 + 3];
      const uint4 o = make_uint4(present_pixel<BG>(v0, b0, b1, b2), present_pixel<BG>(v1, b0, b1, b2), present_pixel<BG>(v2, b0, b1, b2),
                                 present_pixel<BG>(v3, b0, b1, b2));
      if (VEC8) *(uint4 *)(out8 + p0) = o;
      else {
        out8[p0] = o.x;
        out8[p0 + 1] = o.y;
        out8[p0 + 2] = o.z;
        out8[p0 + 3] = o.w;
      }
      if (depth) {
        float4 d;
        if (VECZ) d = *(const float4 *)(depth + p0);
        else d = make_float4(depth[p0], depth[p0 + 1], depth[p0 + 2], depth[p0 + 3]);
        const float4 z = make_float4(present_zw(d.x, n, f, fmn), present_zw(d.y, n, f, fmn), present_zw(d.z, n, f, fmn), present_zw(d.w, n, f, fmn));
        if (VECZ) *(float4 *)(zwin + p0) = z;
        else {
          zwin[p0] = z.x;
          zwin[p0 + 1] = z.y;
          zwin[p0 + 2] = z.z;
          zwin[p0 + 3] = z.w;
        }
      }
    } else {
      for (long long p = p0; p < npix; ++p) {  // the tail: fewer than four pixels
        out8[p] = present_pixel<BG>(in[p], b0, b1, b2);
        if (depth) zwin[p] = present_zw(depth[p], n, f, fmn);
      }
    }
  }
}

// what the rule needs of its arguments: an opaque colour in [0, 1], and for depth a far plane beyond the near plane
static int present_args(smk_ctx *c, const char *who, const float *bg, bool want_depth) {
  if (want_depth && !(c->clip[1] > c->clip[0]))
    FAIL(c, "%s: window depths need a far plane beyond the near plane (clip = %g, %g)", who, c->clip[0], c->clip[1]);
  if (bg)
    for (int k = 0; k < 3; ++k)
      if (!(bg[k] >= 0.0f && bg[k] <= 1.0f)) FAIL(c, "%s: background colour component %d = %g is not in [0, 1]", who, k, bg[k]);
  return 0;
}

// the conversion of one W x H frame, enqueued on s
static int present_launch(smk_ctx *c, const char *who, const void *d_rgba, const void *d_depth, const float *bg, void *d_rgba8, void *d_zwin,
                          hipStream_t s) {
  if (!c->have_camera) FAIL(c, "%s: no camera set (the frame has the window's size)", who);
  if (!d_rgba || !d_rgba8) FAIL(c, "%s: null frame", who);
  if ((d_depth != nullptr) != (d_zwin != nullptr)) FAIL(c, "%s: a view depth and a window-depth output come together or not at all", who);
  if (((uintptr_t)d_rgba & 15) || ((uintptr_t)d_rgba8 & 3)) FAIL(c, "%s: the float frame must be 16-byte aligned, the RGBA8 frame 4-byte aligned", who);
  if (d_depth && (((uintptr_t)d_depth & 3) || ((uintptr_t)d_zwin & 3))) FAIL(c, "%s: depth planes must be 4-byte aligned", who);
  if (present_args(c, who, bg, d_depth != nullptr)) return 1;
  const double n = c->clip[0], f = c->clip[1];
  float b[3] = {0, 0, 0};
  if (bg) memcpy(b, bg, sizeof b);
  const long long npix = (long long)c->W * c->H;
  const bool vec8 = ((uintptr_t)d_rgba8 & 15) == 0;
  const bool vecz = !d_depth || ((((uintptr_t)d_depth | (uintptr_t)d_zwin) & 15) == 0);
  const long long nblocks = std::min<long long>(((npix + 3) / 4 + 255) / 256, 2048);
  const dim3 grid((unsigned)nblocks), block(256);
#define SMK_PRESENT_GO(BG, V8, VZ)                                                                                                   \
  hipLaunchKernelGGL((smk_k_present<BG, V8, VZ>), grid, block, 0, s, (const float4 *)d_rgba, (const float *)d_depth, (uint32_t *)d_rgba8, \
                     (float *)d_zwin, npix, b[0], b[1], b[2], n, f, f - n)
  if (bg) {
    if (vec8 && vecz) SMK_PRESENT_GO(true, true, true);
    else if (vec8) SMK_PRESENT_GO(true, true, false);
    else if (vecz) SMK_PRESENT_GO(true, false, true);
    else SMK_PRESENT_GO(true, false, false);
  } else {
    if (vec8 && vecz) SMK_PRESENT_GO(false, true, true);
    else if (vec8) SMK_PRESENT_GO(false, true, false);
    else if (vecz) SMK_PRESENT_GO(false, false, true);
    else SMK_PRESENT_GO(false, false, false);
  }
#undef SMK_PRESENT_GO
  HIPCHK(c, hipGetLastError());
  return 0;
}

static int event_ready(smk_ctx *c, hipEvent_t *e) {
  if (!*e) HIPCHK(c, hipEventCreate(e));
  return 0;
}

extern "C" int smk_present_device(smk_ctx *c, const void *d_rgba, const void *d_depth, const float *bg, void *d_rgba8, void *d_zwin,
                                  void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  if (event_ready(c, &c->present_ev[0]) || event_ready(c, &c->present_ev[1])) return 1;
  c->present_pending = false;  // (the pair is being recorded again)
  HIPCHK(c, hipEventRecord(c->present_ev[0], s));
  if (present_launch(c, "smk_present_device", d_rgba, d_depth, bg, d_rgba8, d_zwin, s)) return 1;
  HIPCHK(c, hipEventRecord(c->present_ev[1], s));
  c->present_pending = true;  // (smk_get_stat "present_ms" waits for the pair)
  return 0;
}

// smk_get_stat "present_ms": the present kernel of the last frame handed over (or of the last smk_present_device, waited for)
int smk_present_ms(smk_ctx *c, double *value) {
  if (c->present_pending) {
    HIPCHK(c, hipEventSynchronize(c->present_ev[1]));
    HIPCHK(c, hipEventElapsedTime(&c->present_ms, c->present_ev[0], c->present_ev[1]));
    c->present_pending = false;
  }
  *value = c->present_ms;
  return 0;
}

// ------------------------------------------------------------------------------- slots: frames in flight towards the host

bool smk_present_outstanding(const smk_ctx *c) { return c->present[0].outstanding || c->present[1].outstanding; }

static void slot_free_buffers(PresentSlot &S) {
  if (S.d_rgba8) (void)hipFree(S.d_rgba8);
  if (S.d_zwin) (void)hipFree(S.d_zwin);
  if (S.h_rgba8) (void)hipHostFree(S.h_rgba8);
  if (S.h_zwin) (void)hipHostFree(S.h_zwin);
  S.d_rgba8 = nullptr;
  S.d_zwin = nullptr;
  S.h_rgba8 = nullptr;
  S.h_zwin = nullptr;
  S.cap = 0;
}

void smk_present_free(smk_ctx *c) {
  for (PresentSlot &S : c->present) {
    slot_free_buffers(S);
    if (S.d_zscene) (void)hipFree(S.d_zscene);
    for (hipEvent_t e : {S.pev0, S.pev1, S.presented, S.copied})
      if (e) (void)hipEventDestroy(e);
    S = PresentSlot();
  }
  for (hipEvent_t &e : c->present_ev) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  if (c->present_stream) {
    (void)hipStreamSynchronize(c->present_stream);
    (void)hipStreamDestroy(c->present_stream);
    c->present_stream = nullptr;
  }
}

// a slot's buffers for the current window (device and pinned; made on first use, again when the window's pixel count changes)
static int slot_ready(smk_ctx *c, PresentSlot &S, bool scene) {
  const size_t npix = (size_t)c->W * c->H;
  if (npix != S.cap) {
    slot_free_buffers(S);
    HIPCHK(c, hipMalloc((void **)&S.d_rgba8, npix * 4));
    HIPCHK(c, hipMalloc((void **)&S.d_zwin, npix * 4));
    HIPCHK(c, hipHostMalloc((void **)&S.h_rgba8, npix * 4, hipHostMallocDefault));
    HIPCHK(c, hipHostMalloc((void **)&S.h_zwin, npix * 4, hipHostMallocDefault));
    S.cap = npix;
  }
  if (scene && npix > S.zscene_cap) {
    if (S.d_zscene) (void)hipFree(S.d_zscene);
    S.d_zscene = nullptr;
    S.zscene_cap = 0;
    HIPCHK(c, hipMalloc((void **)&S.d_zscene, npix * 4));
    S.zscene_cap = npix;
  }
  if (event_ready(c, &S.pev0) || event_ready(c, &S.pev1) || event_ready(c, &S.presented) || event_ready(c, &S.copied)) return 1;
  if (!c->present_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->present_stream, hipStreamNonBlocking));
  return 0;
}

// the slot's frame on the render stream: ray-march into the context's float frame, present into the slot's device buffers
static int slot_render(smk_ctx *c, const char *who, PresentSlot &S) {
  if (smk_frame_enqueue(c, who, c->d_out, S.want_depth ? c->d_depth : nullptr, S.has_scene ? S.d_zscene : nullptr, S.zkind, c->stream)) return 1;
  S.frame_id = c->frame_id;
  S.ev0 = c->ev0;
  S.ev1 = c->ev1;
  HIPCHK(c, hipEventRecord(S.pev0, c->stream));
  if (present_launch(c, who, c->d_out, S.want_depth ? c->d_depth : nullptr, S.has_bg ? S.bg : nullptr, S.d_rgba8, S.want_depth ? S.d_zwin : nullptr,
                     c->stream))
    return 1;
  HIPCHK(c, hipEventRecord(S.pev1, c->stream));
  return 0;
}

extern "C" int smk_render_present_begin(smk_ctx *c, const float *bg, const float *scene_depth, int zkind, int want_depth, long long *ticket) {
  if (!c) return 1;
  const char *who = "smk_render_present_begin";
  HIPCHK(c, hipSetDevice(c->device));
  if (!ticket) FAIL(c, "%s: null ticket", who);
  if (!c->have_camera) FAIL(c, "%s: no camera set", who);
  if (scene_depth && zkind != SMK_SCENE_VIEW_DEPTH && zkind != SMK_SCENE_WINDOW_DEPTH)
    FAIL(c, "%s: bad scene depth kind %d (SMK_SCENE_VIEW_DEPTH = 0 or SMK_SCENE_WINDOW_DEPTH = 1)", who, zkind);
  if (c->present[0].outstanding && c->present[1].outstanding)
    FAIL(c, "%s: two frames are in flight already (tickets %lld and %lld): end one of them first", who,
         std::min(c->present[0].ticket, c->present[1].ticket), std::max(c->present[0].ticket, c->present[1].ticket));
  const long long t = c->present_ticket + 1;
  PresentSlot &S = c->present[t & 1];  // (tickets alternate: the other slot's pointers stay as they are)
  if (S.outstanding) FAIL(c, "%s: ticket %lld has not been ended and the next frame needs its slot", who, S.ticket);
  if (present_args(c, who, bg, want_depth != 0)) return 1;  // (before anything is enqueued)
  if (smk_frame_buffers(c) || slot_ready(c, S, scene_depth != nullptr)) return 1;
  S.want_depth = want_depth != 0;
  S.has_bg = bg != nullptr;
  if (bg) memcpy(S.bg, bg, sizeof S.bg);
  S.has_scene = scene_depth != nullptr;
  S.zkind = zkind;
  S.npix = (size_t)c->W * c->H;
  // (the host's scene depth is copied at the call, into the slot's own buffer: the frame in the other slot may still read its)
  if (scene_depth) HIPCHK(c, hipMemcpy(S.d_zscene, scene_depth, S.npix * 4, hipMemcpyHostToDevice));
  if (slot_render(c, who, S)) return 1;
  // the copy runs on its own stream behind the present kernel, beside whatever the render stream is given next
  HIPCHK(c, hipEventRecord(S.presented, c->stream));
  HIPCHK(c, hipStreamWaitEvent(c->present_stream, S.presented, 0));
  HIPCHK(c, hipMemcpyAsync(S.h_rgba8, S.d_rgba8, S.npix * 4, hipMemcpyDeviceToHost, c->present_stream));
  if (S.want_depth) HIPCHK(c, hipMemcpyAsync(S.h_zwin, S.d_zwin, S.npix * 4, hipMemcpyDeviceToHost, c->present_stream));
  HIPCHK(c, hipEventRecord(S.copied, c->present_stream));
  c->present_ticket = t;
  S.ticket = t;
  S.outstanding = true;
  *ticket = t;
  return 0;
}

extern "C" int smk_render_present_end(smk_ctx *c, long long ticket, const unsigned char **rgba8, const float **zwin) {
  if (!c) return 1;
  const char *who = "smk_render_present_end";
  HIPCHK(c, hipSetDevice(c->device));
  PresentSlot &S = c->present[ticket & 1];
  if (ticket <= 0 || !S.outstanding || S.ticket != ticket)
    FAIL(c, "%s: ticket %lld is unknown or has been ended already", who, ticket);
  S.outstanding = false;  // (whatever happens below, the ticket is spent)
  HIPCHK(c, hipEventSynchronize(S.copied));
  HIPCHK(c, hipEventElapsedTime(&c->last_ms, S.ev0, S.ev1));
  if (smk_frame_check_status(c, S.frame_id)) {
    // as smk_render: in auto mode the flagged frame is rendered again, by the gather kernel (synchronously, under the
    // context's state of NOW -- a host that moved the camera after `begin` gets the newer pose); otherwise the call fails
    if (c->opt_kernel != 0) return 1;
    const std::string first = c->err;
    ++c->slab_retries;
    if (S.npix != (size_t)c->W * c->H) {
      c->err = first;
      return 1;
    }
    if (slot_render(c, who, S)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->last_kernel != 1 || smk_frame_check_status(c, c->frame_id)) {
      c->err = first;
      return 1;
    }
    HIPCHK(c, hipEventElapsedTime(&c->last_ms, S.ev0, S.ev1));
    HIPCHK(c, hipMemcpy(S.h_rgba8, S.d_rgba8, S.npix * 4, hipMemcpyDeviceToHost));
    if (S.want_depth) HIPCHK(c, hipMemcpy(S.h_zwin, S.d_zwin, S.npix * 4, hipMemcpyDeviceToHost));
    fprintf(stderr, "[smk] %s -- frame rendered again by the gather kernel\n", first.c_str());
  }
  HIPCHK(c, hipEventElapsedTime(&c->present_ms, S.pev0, S.pev1));
  c->present_pending = false;
  c->present_bytes = (double)S.npix * 4 * (S.want_depth ? 2 : 1);
  if (rgba8) *rgba8 = S.h_rgba8;
  if (zwin) *zwin = S.want_depth ? S.h_zwin : nullptr;
  return 0;
}

extern "C" int smk_render_present(smk_ctx *c, const float *bg, const float *scene_depth, int zkind, int want_depth, const unsigned char **rgba8,
                                  const float **zwin) {
  if (!c) return 1;
  long long t = 0;
  if (smk_render_present_begin(c, bg, scene_depth, zkind, want_depth, &t)) return 1;
  return smk_render_present_end(c, t, rgba8, zwin);
}
