// smk_timesteps.hip -- the device-resident time-step cache (DESIGN.md "Time steps").
//
// The reference keeps a ring of `tstepCache` steps in host memory and swaps a cached one in, or reads it from disk
// (MetaVolume::swapTStep / cacheTStep, MetaVolume.cpp:894-958); R8kVolRen3D::draw rebuilds its textures when
// gluvv.volren.timestep moves (R8kVolRen3D.cpp:184-188).  Here the ring lives in HBM: a step is what smk_upload_volume makes
// of a volume (packed voxels, normals, brick summaries), and a switch points the context at another slot.  No voxel is
// copied; the brick flags of the table are made again from the new step's summaries before the next frame, the column
// layout (option "kernel" 3) is rebuilt, and the slice-ring planner forgets the durations it measured on the old step.
//
// Ordering (no host synchronisation on the asynchronous path):
//   - smk_upload_timestep_device enqueues the pack and the brick summaries on the caller's stream and records the slot's
//     `ready` event there; every stream that reads the step (a frame's, the table refresh's) waits for it;
//   - every frame records the slot's `used` event on its stream; an upload into the slot waits for it first;
//   - a kernel that reads a slot and is no frame's (a blend's and a derive's sources, the histogram, the probe, the read-back)
//     waits for the slot's `ready` event and records its `blended` event behind itself: smk_step_read_begin / _end; whatever
//     overwrites a slot waits for that one too;
//   - a blend and a derive write their output slot as an upload does: smk_step_write_begin / _end.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "smk_internal.h"

int smk_step_wait_ready(smk_ctx *c, hipStream_t s) {
  if (c->ts_cur < 0) return 0;
  TimeStep &T = c->ts[c->ts_cur];
  if (!T.ready_pending) return 0;
  if (hipEventQuery(T.ready) == hipSuccess) {
    T.ready_pending = false;  // (long done: no wait to enqueue from now on)
    return 0;
  }
  (void)hipGetLastError();
  HIPCHK(c, hipStreamWaitEvent(s, T.ready, 0));
  return 0;
}

int smk_step_mark_used(smk_ctx *c, hipStream_t s) {
  if (!c->ts_series || c->ts_cur < 0) return 0;  // (a context without a series never overwrites its volume in place)
  TimeStep &T = c->ts[c->ts_cur];
  if (!T.used) HIPCHK(c, hipEventCreateWithFlags(&T.used, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(T.used, s));
  T.used_valid = true;
  return 0;
}

static void free_step(TimeStep &T) {
  if (T.used_valid) (void)hipEventSynchronize(T.used);
  if (T.ready_pending) (void)hipEventSynchronize(T.ready);
  if (T.blended_valid) (void)hipEventSynchronize(T.blended);
  if (T.vox) (void)hipFree(T.vox);
  if (T.nrm) (void)hipFree(T.nrm);
  if (T.mm) (void)hipFree(T.mm);
  if (T.vox_x) (void)hipFree(T.vox_x);
  if (T.derive_st) (void)hipFree(T.derive_st);
  if (T.ready) (void)hipEventDestroy(T.ready);
  if (T.used) (void)hipEventDestroy(T.used);
  if (T.blended) (void)hipEventDestroy(T.blended);
  T = TimeStep();
}

void smk_free_steps(smk_ctx *c) {
  for (TimeStep &T : c->ts) free_step(T);
  c->ts.clear();
  c->ts_cur = -1;
}

void smk_use_step(smk_ctx *c, int k) {
  TimeStep &T = c->ts[(size_t)k];
  c->ts_cur = k;
  c->ts_cur_id = T.id;
  c->d_vox = T.vox;
  c->d_nrm = T.nrm;
  c->d_brick_mm = T.mm;
  c->d_vox_x = T.vox_x_valid ? T.vox_x : nullptr;
  c->bricks3_dirty = true;  // the flags of either table come from this step's summaries
  c->tf_dirty = true;
  c->have_volume = true;
}

// another step (or the current one overwritten): what was derived from the old voxels goes.  The auto mode's measured kernel
// choice stays: it is a property of the configuration, which every step of a series shares.
static void switch_step(smk_ctx *c, int k) {
  smk_use_step(c, k);
  smk_slab_forget_measurements(&c->slab);
  bool layouts = false;
  for (const ColLayout &L : c->cols.lay) layouts |= L.d != nullptr;
  if (layouts) smk_cols_drop_layouts(&c->cols);  // (rebuilt from the new step by its next frame)
}

static int find_step(const smk_ctx *c, int id) {
  for (size_t k = 0; k < c->ts.size(); ++k)
    if (c->ts[k].id == id) return (int)k;
  return -1;
}

int smk_step_slot(const smk_ctx *c, int timestep) {
  if (timestep == SMK_STEP_CURRENT) return c->have_volume ? c->ts_cur : -1;
  return timestep < 0 ? -1 : find_step(c, timestep);
}

// A kernel on stream s that READS slot k and is not a frame: behind the step's upload or blend -- the event stays pending for
// the frames -- and behind the reader before it, on whatever stream, whose `blended` event is recorded again behind this one's
// kernels, so that whatever overwrites the slot waits for every read.
int smk_step_read_begin(smk_ctx *c, int k, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  if (T.ready_pending) HIPCHK(c, hipStreamWaitEvent(s, T.ready, 0));
  if (T.blended_valid) HIPCHK(c, hipStreamWaitEvent(s, T.blended, 0));
  return 0;
}

int smk_step_read_end(smk_ctx *c, int k, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  if (!T.blended) HIPCHK(c, hipEventCreateWithFlags(&T.blended, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(T.blended, s));
  T.blended_valid = true;
  return 0;
}

int step_slot(smk_ctx *c, const char *who, int timestep, int *k) {
  if (!c->have_volume) FAIL(c, "%s: no volume uploaded", who);
  *k = smk_step_slot(c, timestep);
  if (*k < 0) FAIL(c, "%s: time step %d is not cached (upload it with smk_upload_timestep)", who, timestep);
  return 0;
}

static size_t bytes_per_step(const smk_ctx *c) {
  return c->vox_bytes + 16 + smk_step_nrm_bytes(c) + (size_t)c->nbr[0] * c->nbr[1] * c->nbr[2] * sizeof(float4);
}

extern "C" int smk_set_timestep_cache(smk_ctx *c, int nsteps) {
  if (!c) return 1;
  if (nsteps < 1) FAIL(c, "smk_set_timestep_cache: capacity %d: the cache holds at least the current step", nsteps);
  HIPCHK(c, hipSetDevice(c->device));
  c->ts_series = true;
  if (!c->have_volume) {
    c->ts_cap = nsteps;
    return 0;
  }
  int held = 0;
  for (const TimeStep &T : c->ts) held += T.vox != nullptr;
  if (nsteps > held) {
    const size_t per = bytes_per_step(c), need = per * (size_t)(nsteps - held);
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    if (need > fr)
      FAIL(c, "smk_set_timestep_cache: %d steps do not fit: %zu bytes per step, %zu bytes more needed, %zu free", nsteps, per, need, fr);
  }
  // the slots in the order they were written; the current step and the newest others stay, in that order from slot 0
  std::vector<int> order;
  for (size_t k = 0; k < c->ts.size(); ++k)
    if (c->ts[k].id >= 0) order.push_back((int)k);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return c->ts[(size_t)a].written < c->ts[(size_t)b].written; });
  std::vector<int> keep;
  if (c->ts_cur >= 0) keep.push_back(c->ts_cur);
  for (int i = (int)order.size() - 1; i >= 0 && (int)keep.size() < nsteps; --i)
    if (order[(size_t)i] != c->ts_cur) keep.push_back(order[(size_t)i]);
  std::sort(keep.begin(), keep.end(), [&](int a, int b) { return c->ts[(size_t)a].written < c->ts[(size_t)b].written; });
  std::vector<TimeStep> ring((size_t)nsteps);
  int cur = -1;
  for (size_t i = 0; i < keep.size(); ++i) {
    if (keep[i] == c->ts_cur) cur = (int)i;
    ring[i] = c->ts[(size_t)keep[i]];
    c->ts[(size_t)keep[i]] = TimeStep();
  }
  for (TimeStep &T : c->ts) free_step(T);  // the evicted steps (after the frames that read them)
  // (slots that held no step keep no buffers: a later upload makes them)
  c->ts.swap(ring);
  c->ts_cap = nsteps;
  c->ts_cur = cur;
  return 0;
}

// the slot a new step takes: an empty one, else the one after the slot written last (cacheTStep's oldTSpos), never the
// current step's
static int next_slot(const smk_ctx *c) {
  for (size_t k = 0; k < c->ts.size(); ++k)
    if (c->ts[k].id < 0) return (int)k;
  int last = 0;
  for (size_t k = 0; k < c->ts.size(); ++k)
    if (c->ts[k].written > c->ts[(size_t)last].written) last = (int)k;
  int k = (last + 1) % (int)c->ts.size();
  if (k == c->ts_cur) k = (k + 1) % (int)c->ts.size();
  return k;
}

static int upload_step(smk_ctx *c, const char *who, int id, const smk_volume_desc *b, int nb, int nelts, smk_dtype dtype,
                       smk_datamode dmode, bool on_device, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (id < 0) FAIL(c, "%s: time step %d: ids are >= 0", who, id);
  SmkVolGeom g;
  if (smk_volume_geometry(c, who, b, nb, nelts, dtype, dmode, g)) return 1;
  c->ts_series = true;
  if (c->have_volume) {  // every step has the geometry of the first upload
    if (g.N[0] != c->N[0] || g.N[1] != c->N[1] || g.N[2] != c->N[2])
      FAIL(c, "%s: time step %d: sizes %dx%dx%d differ from the series' %dx%dx%d", who, id, g.N[0], g.N[1], g.N[2], c->N[0], c->N[1], c->N[2]);
    if (g.fs[0] != c->fsize[0] || g.fs[1] != c->fsize[1] || g.fs[2] != c->fsize[2])
      FAIL(c, "%s: time step %d: extents %g x %g x %g differ from the series' %g x %g x %g", who, id, g.fs[0], g.fs[1], g.fs[2],
           c->fsize[0], c->fsize[1], c->fsize[2]);
    if (g.nelts != c->nelts) FAIL(c, "%s: time step %d: nelts %d differs from the series' %d", who, id, g.nelts, c->nelts);
    if (g.dtype != c->dtype) FAIL(c, "%s: time step %d: dtype %d differs from the series' %d", who, id, g.dtype, c->dtype);
    if (g.dmode != c->dmode) FAIL(c, "%s: time step %d: datamode %d differs from the series' %d", who, id, g.dmode, c->dmode);
    if (g.grad != c->have_normals)
      FAIL(c, "%s: time step %d: normals %s, the series' %s", who, id, g.grad ? "present" : "absent", c->have_normals ? "present" : "absent");
  }
  int k = c->have_volume ? find_step(c, id) : -1;
  if (k < 0) {
    if (!c->have_volume) {  // the first step: it sets the geometry, and is the current one
      smk_set_geometry(c, g);
      c->ts.assign((size_t)c->ts_cap, TimeStep());
      c->ts_cur = -1;
      c->tune_choice.clear();
      c->tune_sig = 0;
    } else if (c->ts.size() == 1)
      FAIL(c, "%s: time step %d: the cache holds one step, the current one (%d); smk_set_timestep_cache sets more", who, id, c->ts_cur_id);
    k = next_slot(c);
  }
  TimeStep &T = c->ts[(size_t)k];
  const hipStream_t s = on_device ? (stream ? (hipStream_t)stream : c->stream) : nullptr;
  // the slot's old contents: the frames that read them, and an upload still writing them, come first
  if (T.used_valid) {
    if (s) HIPCHK(c, hipStreamWaitEvent(s, T.used, 0));
    else HIPCHK(c, hipEventSynchronize(T.used));
  }
  if (T.ready_pending) {
    if (s) HIPCHK(c, hipStreamWaitEvent(s, T.ready, 0));
    else HIPCHK(c, hipEventSynchronize(T.ready));
    T.ready_pending = false;
  }
  if (T.blended_valid) {  // ... and a blend still reading them (smk_blend_timesteps)
    if (s) HIPCHK(c, hipStreamWaitEvent(s, T.blended, 0));
    else HIPCHK(c, hipEventSynchronize(T.blended));
    T.blended_valid = false;  // (whoever writes the slot next is ordered behind this upload)
  }
  T.id = -1;  // (until it holds the new step)
  if (smk_alloc_step(c, g, T)) return 1;
  if (smk_pack_step(c, who, g, b, nb, on_device, T, s)) return 1;
  T.id = id;
  T.written = ++c->ts_written;
  if (s) {
    if (!T.ready) HIPCHK(c, hipEventCreateWithFlags(&T.ready, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(T.ready, s));
    T.ready_pending = true;
  }
  if (c->ts_cur < 0) smk_use_step(c, k);
  else if (k == c->ts_cur) switch_step(c, k);  // the current step overwritten in place
  return 0;
}

int smk_step_output_slot(const smk_ctx *c, int id, int ka, int kb, int *need) {
  const int k = find_step(c, id);
  if (k >= 0) return k;  // a cached step is overwritten in place
  const int cur = c->ts_cur;
  *need = 1 + (ka >= 0 ? 1 : 0) + (kb >= 0 && kb != ka ? 1 : 0) + (cur >= 0 && cur != ka && cur != kb ? 1 : 0);
  if ((int)c->ts.size() < *need) return -1;
  int n = next_slot(c);
  while (n == ka || n == kb || n == cur) n = (n + 1) % (int)c->ts.size();
  return n;
}

int smk_step_write_begin(smk_ctx *c, int k, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  // the slot's old contents: the frames, blends and reads that use them, and an upload still writing them
  if (T.used_valid) HIPCHK(c, hipStreamWaitEvent(s, T.used, 0));
  if (T.blended_valid) {
    HIPCHK(c, hipStreamWaitEvent(s, T.blended, 0));
    T.blended_valid = false;  // (whoever writes the slot next is ordered behind this write)
  }
  if (T.ready_pending) {
    HIPCHK(c, hipStreamWaitEvent(s, T.ready, 0));
    T.ready_pending = false;
  }
  T.id = -1;  // (until it holds the new step)
  SmkVolGeom g;  // the series' buffers (the writer fills the pad column of a padded box itself: a blend with 0 blended with 0)
  g.vox_bytes = c->vox_bytes;
  g.nrm_bytes = smk_step_nrm_bytes(c);
  g.mm_bytes = (size_t)c->nbr[0] * c->nbr[1] * c->nbr[2] * sizeof(float4);
  return smk_alloc_step(c, g, T);
}

int smk_step_write_end(smk_ctx *c, int k, int id, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  T.vox_x_valid = false;
  T.id = id;
  T.written = ++c->ts_written;
  if (!T.ready) HIPCHK(c, hipEventCreateWithFlags(&T.ready, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(T.ready, s));
  T.ready_pending = true;
  if (k == c->ts_cur) switch_step(c, k);  // the current step overwritten in place
  return 0;
}

extern "C" int smk_upload_timestep(smk_ctx *c, int timestep, const smk_volume_desc *bricks, int n_bricks, int nelts, smk_dtype dtype,
                                   smk_datamode dmode) {
  return upload_step(c, "smk_upload_timestep", timestep, bricks, n_bricks, nelts, dtype, dmode, false, nullptr);
}

extern "C" int smk_upload_timestep_device(smk_ctx *c, int timestep, const smk_volume_desc *bricks, int n_bricks, int nelts,
                                          smk_dtype dtype, smk_datamode dmode, void *stream) {
  return upload_step(c, "smk_upload_timestep_device", timestep, bricks, n_bricks, nelts, dtype, dmode, true, stream);
}

extern "C" int smk_select_timestep(smk_ctx *c, int timestep) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  c->ts_series = true;
  if (!c->have_volume) FAIL(c, "smk_select_timestep: no volume uploaded");
  const int k = find_step(c, timestep);
  if (k < 0) FAIL(c, "smk_select_timestep: time step %d is not cached (upload it with smk_upload_timestep)", timestep);
  if (k != c->ts_cur) switch_step(c, k);
  return 0;
}

extern "C" int smk_get_timesteps(smk_ctx *c, int *current, int *ids_out, int cap, int *n) {
  if (!c) return 1;
  std::vector<const TimeStep *> held;
  for (const TimeStep &T : c->ts)
    if (T.id >= 0) held.push_back(&T);
  std::sort(held.begin(), held.end(), [](const TimeStep *a, const TimeStep *b) { return a->written < b->written; });
  if (current) *current = c->have_volume ? c->ts_cur_id : -1;
  if (n) *n = (int)held.size();
  if (ids_out)
    for (int i = 0; i < cap && i < (int)held.size(); ++i) ids_out[i] = held[(size_t)i]->id;
  return 0;
}

// ------------------------------------------------------------------------------- fractional time (smk_blend_timesteps)
//
// A blended step is a step: the packed voxels of two slots blended field by field into a third, then the brick summaries
// of the result, as after an upload.  The arithmetic is smk.h's: u = 1 - w once on the host, r = (u * x) + (w * y) in fp32
// with one rounding per operation (two products, one sum: the build's -ffp-contract=off, restated below), a float field
// stores r, an integer field min((int)(r + 0.5f), top).
#pragma clang fp contract(off)

namespace {

// What the four words of a 16-byte unit hold (smk_packed.h): FORM is the voxels' smk_dtype -- SMK_U8, all bytes, is also the
// form of the separate normals buffer; SMK_U16 is two 16-bit channels, then bytes -- with f32 split by what .w holds:
enum { TB_F32N = SMK_F32,  // an f32 voxel of up to three channels: three floats, the normal bytes in .w
       TB_F32C = 3 };      // a four-channel f32 voxel: four floats

__device__ __forceinline__ uint32_t tb_int(uint32_t x, uint32_t y, float u, float w, int top) {
  const float r = (u * (float)x) + (w * (float)y);
  return (uint32_t)min((int)(r + 0.5f), top);
}

__device__ __forceinline__ uint32_t tb_bytes(uint32_t x, uint32_t y, float u, float w) {
  uint32_t o = 0;
#pragma unroll
  for (int k = 0; k < 32; k += 8) o |= tb_int((x >> k) & 255u, (y >> k) & 255u, u, w, 255) << k;
  return o;
}

__device__ __forceinline__ uint32_t tb_shorts(uint32_t x, uint32_t y, float u, float w) {
  return tb_int(x & 65535u, y & 65535u, u, w, 65535) | (tb_int(x >> 16, y >> 16, u, w, 65535) << 16);
}

__device__ __forceinline__ uint32_t tb_float(uint32_t x, uint32_t y, float u, float w) {
  return __float_as_uint((u * __uint_as_float(x)) + (w * __uint_as_float(y)));
}

template <int FORM>
__device__ __forceinline__ uint4 tb_unit(const uint4 x, const uint4 y, float u, float w) {
  uint4 o;
  if (FORM == SMK_U8) {
    o.x = tb_bytes(x.x, y.x, u, w); o.y = tb_bytes(x.y, y.y, u, w); o.z = tb_bytes(x.z, y.z, u, w); o.w = tb_bytes(x.w, y.w, u, w);
  } else if (FORM == SMK_U16) {
    o.x = tb_shorts(x.x, y.x, u, w); o.y = tb_bytes(x.y, y.y, u, w); o.z = tb_shorts(x.z, y.z, u, w); o.w = tb_bytes(x.w, y.w, u, w);
  } else {
    o.x = tb_float(x.x, y.x, u, w); o.y = tb_float(x.y, y.y, u, w); o.z = tb_float(x.z, y.z, u, w);
    o.w = FORM == TB_F32N ? tb_bytes(x.w, y.w, u, w) : tb_float(x.w, y.w, u, w);
  }
  return o;
}

// One linear pass over `units` 16-byte units: out = (1 - w) a + w b per stored field.  A workgroup takes TB_PER runs of 256
// consecutive units per turn (a wave's load or store instruction covers 1 KiB), and every load of a turn is issued before
// its arithmetic: 2 * TB_PER * 16 bytes per lane in flight.  The grid is capped and strides over the rest.
constexpr int TB_PER = 4;
constexpr unsigned TB_MAX_BLOCKS = 2048;  // 8 workgroups for each of 256 CUs

template <int FORM>
__global__ __launch_bounds__(256) void smk_k_blend_steps(const uint4 *__restrict__ a, const uint4 *__restrict__ b, uint4 *__restrict__ out,
                                                          size_t units, float u, float w) {
  const size_t turn = (size_t)256 * TB_PER, stride = (size_t)gridDim.x * turn;
  for (size_t base = (size_t)blockIdx.x * turn + threadIdx.x; base < units; base += stride) {
    uint4 x[TB_PER], y[TB_PER];
#pragma unroll
    for (int j = 0; j < TB_PER; ++j) {
      const size_t i = base + (size_t)j * 256;
      if (i < units) {
        x[j] = a[i];
        y[j] = b[i];
      }
    }
#pragma unroll
    for (int j = 0; j < TB_PER; ++j) {
      const size_t i = base + (size_t)j * 256;
      if (i < units) out[i] = tb_unit<FORM>(x[j], y[j], u, w);
    }
  }
}

// the last n < 4 words of a buffer of packed normals
__global__ __launch_bounds__(64) void smk_k_blend_words(const uint32_t *a, const uint32_t *b, uint32_t *out, int n, float u, float w) {
  if ((int)threadIdx.x < n) out[threadIdx.x] = tb_bytes(a[threadIdx.x], b[threadIdx.x], u, w);
}

template <int FORM>
hipError_t launch_blend(const void *a, const void *b, void *out, size_t units, float u, float w, hipStream_t s) {
  if (!units) return hipSuccess;
  const size_t turn = (size_t)256 * TB_PER, blocks = std::min((units + turn - 1) / turn, (size_t)TB_MAX_BLOCKS);
  hipLaunchKernelGGL(smk_k_blend_steps<FORM>, dim3((unsigned)blocks), dim3(256), 0, s, (const uint4 *)a, (const uint4 *)b, (uint4 *)out, units, u,
                     w);
  return hipGetLastError();
}

}  // namespace

extern "C" int smk_blend_timesteps(smk_ctx *c, int step_a, int step_b, float w, int step_out, void *stream) {
  if (!c) return 1;
  const char *who = "smk_blend_timesteps";
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_volume) FAIL(c, "%s: no volume uploaded", who);
  const int ka = find_step(c, step_a), kb = find_step(c, step_b);
  if (step_a < 0 || ka < 0) FAIL(c, "%s: time step %d (a) is not cached", who, step_a);
  if (step_b < 0 || kb < 0) FAIL(c, "%s: time step %d (b) is not cached", who, step_b);
  if (step_out < 0) FAIL(c, "%s: output time step %d: ids are >= 0", who, step_out);
  if (step_out == step_a || step_out == step_b)
    FAIL(c, "%s: output time step %d is also a source: the blend has no in-place form", who, step_out);
  if (!(w >= 0.0f && w <= 1.0f)) FAIL(c, "%s: weight %g is not in [0, 1] (no extrapolation)", who, (double)w);
  c->ts_series = true;
  // a cached output's own slot, else one by next_slot's rule that is neither source's nor the current step's: the sources,
  // the current step and the output are 3 or 4 slots (one less where a and b are the same step)
  int need = 0;
  const int k = smk_step_output_slot(c, step_out, ka, kb, &need);
  if (k < 0)
    FAIL(c, "%s: the cache holds %d steps: the two sources and the output need three slots, four when the current step (%d) is a fourth "
            "(here %d); smk_set_timestep_cache sets more", who, (int)c->ts.size(), c->ts_cur_id, need);
  TimeStep &A = c->ts[(size_t)ka], &B = c->ts[(size_t)kb], &T = c->ts[(size_t)k];
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  // the sources: behind their uploads (or blends) and their last reader; their `blended` events are recorded again below
  if (smk_step_read_begin(c, ka, s) || smk_step_read_begin(c, kb, s)) return 1;
  // the output slot's old contents: the frames and the blends that read them, and an upload still writing them; its buffers
  if (smk_step_write_begin(c, k, s)) return 1;
  const size_t nst = (size_t)c->D[0] * c->D[1] * c->D[2];
  // the stored box in 16-byte units (a whole number of them: smk_packed.h); the 16 bytes behind the box are not touched
  const float u = 1.0f - w;
  const size_t units = c->vox_bytes / 16;
  if (c->dtype == SMK_U8) HIPCHK(c, launch_blend<SMK_U8>(A.vox, B.vox, T.vox, units, u, w, s));
  else if (c->dtype == SMK_U16) HIPCHK(c, launch_blend<SMK_U16>(A.vox, B.vox, T.vox, units, u, w, s));
  else if (c->nelts <= 3) HIPCHK(c, launch_blend<TB_F32N>(A.vox, B.vox, T.vox, units, u, w, s));
  else HIPCHK(c, launch_blend<TB_F32C>(A.vox, B.vox, T.vox, units, u, w, s));
  if (smk_step_nrm_bytes(c)) {
    // the separate normals of four-channel f32, a word per voxel, in the byte form: the whole units, then the words that
    // are left when the voxel count (odd sizes are allowed for f32) is no multiple of four
    HIPCHK(c, launch_blend<SMK_U8>(A.nrm, B.nrm, T.nrm, nst / 4, u, w, s));
    if (nst % 4) {
      const size_t done = nst / 4 * 4;
      hipLaunchKernelGGL(smk_k_blend_words, dim3(1), dim3(64), 0, s, A.nrm + done, B.nrm + done, T.nrm + done, (int)(nst % 4), u, w);
      HIPCHK(c, hipGetLastError());
    }
  }
  HIPCHK(c, smk_bricks_minmax(T.vox, c->dtype, c->D, c->nbr, T.mm, s));
  if (smk_step_write_end(c, k, step_out, s)) return 1;  // (the output's `ready`; the current step overwritten in place)
  if (smk_step_read_end(c, ka, s) || smk_step_read_end(c, kb, s)) return 1;  // whatever overwrites a source slot comes after these reads
  ++c->tblend_count;
  return 0;
}
