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
//   - a kernel that reads a slot and is no frame's (a producer's sources, the histogram, the read-back) runs inside
//     smk_step_read: behind the slot's `ready` event and the reader before it, with the slot's `nonframe_read` event recorded
//     behind it, also when one of its launches failed.  The probe waits alike and synchronises;
//   - whatever writes a slot (an upload, a producer) first waits for its `used`, `ready` and `nonframe_read` events;
//   - a producer (blend, derive, merge: kernels that make a step from what is on the device) runs inside smk_step_produce,
//     which is all of the above once: the output slot by the ring's rule, the sources' and the output slot's waits, the
//     producer's kernels, the brick summaries, `ready`, the sources' read events.
#include <limits.h>

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
  if (T.nonframe_read_valid) (void)hipEventSynchronize(T.nonframe_read);
  if (T.vox) (void)hipFree(T.vox);
  if (T.nrm) (void)hipFree(T.nrm);
  if (T.mm) (void)hipFree(T.mm);
  if (T.vox_x) (void)hipFree(T.vox_x);
  if (T.pass1_words) (void)hipFree(T.pass1_words);
  if (T.ready) (void)hipEventDestroy(T.ready);
  if (T.used) (void)hipEventDestroy(T.used);
  if (T.nonframe_read) (void)hipEventDestroy(T.nonframe_read);
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

// A kernel on stream s that READS slot k and is not a frame: behind the step's writer -- the event stays pending for the
// frames -- and behind the reader before it, on whatever stream, whose `nonframe_read` event smk_step_read records again behind
// this one's kernels, so that whatever overwrites the slot waits for every read.
int smk_step_read_begin(smk_ctx *c, int k, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  if (T.ready_pending) HIPCHK(c, hipStreamWaitEvent(s, T.ready, 0));
  if (T.nonframe_read_valid) HIPCHK(c, hipStreamWaitEvent(s, T.nonframe_read, 0));
  return 0;
}

static int read_end(smk_ctx *c, int k, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  if (!T.nonframe_read) HIPCHK(c, hipEventCreateWithFlags(&T.nonframe_read, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(T.nonframe_read, s));
  T.nonframe_read_valid = true;
  return 0;
}

int smk_step_read(smk_ctx *c, int ka, int kb, hipStream_t s, const std::function<int()> &launches) {
  int rc = (ka >= 0 && smk_step_read_begin(c, ka, s)) || (kb >= 0 && smk_step_read_begin(c, kb, s));
  if (!rc) rc = launches();
  const std::string why = c->err;  // every return of a reader passes here; the first failure is the one reported
  bool lost = ka >= 0 && read_end(c, ka, s);
  if (kb >= 0 && read_end(c, kb, s)) lost = true;
  if (rc) c->err = why;
  return rc || lost;
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

// A writer of slot T comes behind the slot's old contents: the frames that read them, a writer still making them and their
// last reader that is no frame.  Stream s waits, or without one (a host upload) the host.  The slot is empty from here on
static int wait_old_contents(smk_ctx *c, TimeStep &T, hipStream_t s) {
  const auto wait = [s](hipEvent_t e) { return s ? hipStreamWaitEvent(s, e, 0) : hipEventSynchronize(e); };
  if (T.used_valid) HIPCHK(c, wait(T.used));
  if (T.ready_pending) {
    HIPCHK(c, wait(T.ready));
    T.ready_pending = false;
  }
  if (T.nonframe_read_valid) {
    HIPCHK(c, wait(T.nonframe_read));
    T.nonframe_read_valid = false;
  }
  T.id = -1;
  return 0;
}

// ... and with its writer enqueued slot k holds step `id`: `ready` on s (a host upload needs none); the series' first step,
// or the current one overwritten in place, is what the next frame shows
static int step_written(smk_ctx *c, int k, int id, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  T.id = id;
  T.written = ++c->ts_written;
  if (s) {
    if (!T.ready) HIPCHK(c, hipEventCreateWithFlags(&T.ready, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(T.ready, s));
    T.ready_pending = true;
  }
  if (c->ts_cur < 0) smk_use_step(c, k);
  else if (k == c->ts_cur) switch_step(c, k);
  return 0;
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
  if (wait_old_contents(c, T, s)) return 1;
  if (smk_alloc_step(c, g, T)) return 1;
  if (smk_pack_step(c, who, g, b, nb, on_device, T, s)) return 1;
  return step_written(c, k, id, s);
}

// the slot step `id` takes: a cached id's own (overwritten in place), else one by next_slot's rule that is neither slot ka
// nor kb (the sources; -1: none) nor the current step's; -1 when the ring has fewer than *need slots
static int output_slot(const smk_ctx *c, int id, int ka, int kb, int *need) {
  const int k = find_step(c, id);
  if (k >= 0) return k;
  const int cur = c->ts_cur;
  *need = 1 + (ka >= 0 ? 1 : 0) + (kb >= 0 && kb != ka ? 1 : 0) + (cur >= 0 && cur != ka && cur != kb ? 1 : 0);
  if ((int)c->ts.size() < *need) return -1;
  int n = next_slot(c);
  while (n == ka || n == kb || n == cur) n = (n + 1) % (int)c->ts.size();
  return n;
}

int smk_step_produce(smk_ctx *c, const char *who, int id, int ka, int kb, hipStream_t s, const StepLaunches &launches) {
  c->ts_series = true;
  int need = 0;
  const int k = output_slot(c, id, ka, kb, &need);
  if (k < 0) {
    const int held = (int)c->ts.size(), cur = c->ts_cur_id;
    if (ka >= 0 && kb >= 0)
      FAIL(c, "%s: the cache holds %d steps: the two sources and the output need three slots, four when the current step (%d) is a fourth "
              "(here %d); smk_set_timestep_cache sets more", who, held, cur, need);
    if (ka >= 0 || kb >= 0)
      FAIL(c, "%s: the cache holds %d steps: the source and the output need two slots, three when the current step (%d) is a third "
              "(here %d); smk_set_timestep_cache sets more", who, held, cur, need);
    FAIL(c, "%s: time step %d: the cache holds one step, the current one (%d); smk_set_timestep_cache sets more", who, id, cur);
  }
  return smk_step_read(c, ka, kb, s, [&]() -> int {
    TimeStep &T = c->ts[(size_t)k];
    if (wait_old_contents(c, T, s)) return 1;
    SmkVolGeom g;  // the series' buffers (the kernels fill the pad column of a padded box themselves)
    g.vox_bytes = c->vox_bytes;
    g.nrm_bytes = smk_step_nrm_bytes(c);
    g.mm_bytes = (size_t)c->nbr[0] * c->nbr[1] * c->nbr[2] * sizeof(float4);
    if (smk_alloc_step(c, g, T)) return 1;
    // what is valid of the result: what is valid of every source (a blend), all of the stored box without one (dense
    // arrays); a sharded stencil producer narrows it in its `launches` (smk_step_shard_done)
    T.valid_halo = c->halo;
    for (int a = 0; a < 3; ++a) {
      T.vlo[a] = c->O[a];
      T.vhi[a] = std::min(c->O[a] + c->D[a], c->N[a]);
    }
    for (const int ks : {ka, kb}) {
      if (ks < 0) continue;
      const TimeStep &S = c->ts[(size_t)ks];
      T.valid_halo = std::min(T.valid_halo, S.valid_halo);
      for (int a = 0; a < 3; ++a) {
        T.vlo[a] = std::max(T.vlo[a], S.vlo[a]);
        T.vhi[a] = std::min(T.vhi[a], S.vhi[a]);
      }
    }
    if (launches(T, ka >= 0 ? &c->ts[(size_t)ka] : nullptr, kb >= 0 ? &c->ts[(size_t)kb] : nullptr)) return 1;
    HIPCHK(c, smk_bricks_minmax(T.vox, c->dtype, c->D, c->nbr, T.mm, s));
    T.vox_x_valid = false;
    return step_written(c, k, id, s);
  });
}

int smk_step_rewrite(smk_ctx *c, int k, hipStream_t s, const std::function<int(TimeStep &)> &launches) {
  c->ts_series = true;
  TimeStep &T = c->ts[(size_t)k];
  const int id = T.id;
  const int waited = wait_old_contents(c, T, s);
  T.id = id;  // (the slot is not emptied: the step stays what it was, with more of it valid)
  if (waited) return 1;
  T.vox_x_valid = false;
  int rc = launches(T);
  if (!rc) {
    const hipError_t e = smk_bricks_minmax(T.vox, c->dtype, c->D, c->nbr, T.mm, s);
    if (e != hipSuccess) {
      c->err = std::string("smk_bricks_minmax failed: ") + hipGetErrorString(e);
      rc = 1;
    }
  }
  const std::string why = c->err;
  if (!T.ready) HIPCHK(c, hipEventCreateWithFlags(&T.ready, hipEventDisableTiming));
  HIPCHK(c, hipEventRecord(T.ready, s));
  T.ready_pending = true;
  if (k == c->ts_cur) switch_step(c, k);
  if (rc) c->err = why;
  return rc;
}

int smk_step_stencil_refusals(smk_ctx *c, const StencilEntry &E, int step_out, const int *step_src, int *ksrc) {
  const char *who = E.who;
  if (!c->have_volume) FAIL(c, "%s: no volume uploaded", who);
  if (c->nranks > 1) FAIL(c, "%s: a sharded context (%d ranks): %s", who, c->nranks, E.sharded_why);
  if (!E.nelts_why.empty()) FAIL(c, "%s: %s", who, E.nelts_why.c_str());
  // what the kernels take for granted of an unsharded context's stored box (smk_volume_geometry): it starts at voxel 0, is
  // the volume in z, and is wider than the volume only by the pad column and row of 8-byte voxels, to an even D[0]
  const bool wide = c->dtype == SMK_F32;
  if (c->O[0] || c->O[1] || c->O[2] || c->D[2] != c->N[2] || c->D[0] < c->N[0] || c->D[1] < c->N[1] || c->D[0] > c->N[0] + 1 ||
      c->D[1] > c->N[1] + 1 || (wide && (c->D[0] != c->N[0] || c->D[1] != c->N[1])) || (!wide && (c->D[0] & 1)))
    FAIL(c, "%s: internal: the stored box %dx%dx%d at %d,%d,%d is not the volume %dx%dx%d with its pad", who, c->D[0], c->D[1], c->D[2], c->O[0],
         c->O[1], c->O[2], c->N[0], c->N[1], c->N[2]);
  if (c->N[0] < 3 || c->N[1] < 3 || c->N[2] < 3)
    FAIL(c, "%s: a %dx%dx%d volume has no interior voxel (dims >= 3, as %s)", who, c->N[0], c->N[1], c->N[2], E.prep_entry);
  if (!step_src && step_out < 0) FAIL(c, "%s: time step %d: ids are >= 0", who, step_out);
  if (!step_src) return 0;
  *ksrc = *step_src < 0 ? -1 : smk_step_slot(c, *step_src);
  if (*ksrc < 0) FAIL(c, "%s: time step %d (the source) is not cached", who, *step_src);
  if (step_out < 0) FAIL(c, "%s: output time step %d: ids are >= 0", who, step_out);
  if (step_out == *step_src) FAIL(c, "%s: output time step %d is also the source: the stencil has no in-place form", who, step_out);
  return 0;
}

// ---------------------------------------------------------------------- the stencil producers on a shard: what is valid

// a face of the SOURCE's valid box that is a face of the volume loses nothing to a stencil: beyond it lies no voxel.  (Not
// a face of the stored box: a block step with ghosts narrower than option "halo" is valid from voxel 2 of a box stored from 0.)
static bool volume_face(const smk_ctx *c, const TimeStep &src, int a, int hi) { return hi ? src.vhi[a] >= c->N[a] : src.vlo[a] == 0; }

int smk_step_shown_halo(const smk_ctx *c) { return c->ts_cur >= 0 ? c->ts[(size_t)c->ts_cur].valid_halo : c->halo; }

// what the shard and the block entries refuse of the context before they look at a source
static int shard_context_refusals(smk_ctx *c, const StencilEntry &E) {
  const char *who = E.who;
  if (!c->have_volume) FAIL(c, "%s: no volume uploaded", who);
  if (!E.nelts_why.empty()) FAIL(c, "%s: %s", who, E.nelts_why.c_str());
  // what the shard kernels take for granted of a stored box (smk_volume_geometry): it lies in the volume but for the pad
  // column and row of 8-byte voxels, which exist only behind the volume's last voxel, it has an even D[0] then, and it holds
  // the region
  const bool wide = c->dtype == SMK_F32;
  bool fits = wide || !(c->D[0] & 1);
  for (int a = 0; a < 3; ++a) {
    const int pad = !wide && a < 2 ? 1 : 0;
    fits = fits && c->O[a] >= 0 && c->D[a] >= 1 && c->O[a] + c->D[a] <= c->N[a] + pad && c->g0[a] >= c->O[a] && c->g1[a] >= c->g0[a] &&
           c->g1[a] <= std::min(c->O[a] + c->D[a], c->N[a]);
  }
  if (!fits)
    FAIL(c, "%s: internal: the stored box %dx%dx%d at %d,%d,%d does not hold its region inside the volume %dx%dx%d", who, c->D[0], c->D[1], c->D[2],
         c->O[0], c->O[1], c->O[2], c->N[0], c->N[1], c->N[2]);
  if (c->N[0] < 3 || c->N[1] < 3 || c->N[2] < 3)
    FAIL(c, "%s: a %dx%dx%d volume has no interior voxel (dims >= 3, as %s)", who, c->N[0], c->N[1], c->N[2], E.prep_entry);
  return 0;
}

int smk_step_shard_refusals(smk_ctx *c, const StencilEntry &E, int reach, int step_src, const int *step_out, int *ksrc) {
  const char *who = E.who;
  if (shard_context_refusals(c, E)) return 1;
  *ksrc = step_src < 0 ? -1 : smk_step_slot(c, step_src);
  if (*ksrc < 0) FAIL(c, "%s: time step %d (the source) is not cached", who, step_src);
  if (step_out) {
    if (*step_out < 0) FAIL(c, "%s: output time step %d: ids are >= 0", who, *step_out);
    if (*step_out == step_src) FAIL(c, "%s: output time step %d is also the source: the stencil has no in-place form", who, *step_out);
  }
  const int have = c->ts[(size_t)*ksrc].valid_halo;
  if (c->nranks > 1 && have < reach + 1)  // (every rank of a sharded series alike, whatever its own box is cut by)
    FAIL(c, "%s: time step %d (the source) has a valid halo of %d voxels, the stencil reaches %d and the result keeps one for a frame: a valid "
            "halo >= %d is needed (option 'halo', set before upload, less the reach of every stencil the step went through)", who, step_src, have,
         reach, reach + 1);
  return 0;
}

void smk_step_shard_box(const smk_ctx *c, const TimeStep &src, int reach, SmkShardBox &B) {
  for (int a = 0; a < 3; ++a) {
    B.O[a] = c->O[a];
    B.r0[a] = c->g0[a] - c->O[a];
    B.r1[a] = c->g1[a] - c->O[a];
    B.v0[a] = (volume_face(c, src, a, 0) ? src.vlo[a] : src.vlo[a] + reach) - c->O[a];
    B.v1[a] = (volume_face(c, src, a, 1) ? src.vhi[a] : src.vhi[a] - reach) - c->O[a];
  }
}

void smk_step_shard_done(const smk_ctx *c, const TimeStep &src, int reach, const SmkShardBox &B, TimeStep &out) {
  out.valid_halo = c->nranks > 1 ? src.valid_halo - reach : src.valid_halo;
  for (int a = 0; a < 3; ++a) {
    out.vlo[a] = B.v0[a] + c->O[a];
    out.vhi[a] = B.v1[a] + c->O[a];
  }
}

// ---------------------------------------------------------------------- blocks of a decomposed simulation: what is valid

int smk_block_view(smk_ctx *c, const char *who, const smk_block *b, SmkBlockView &V) {
  if (!b) FAIL(c, "%s: block is NULL", who);
  for (int a = 0; a < 3; ++a)
    if (b->size[a] <= 0) FAIL(c, "%s: block size %dx%dx%d: sizes are > 0", who, b->size[0], b->size[1], b->size[2]);
  V.py = b->pitch_y ? b->pitch_y : (long long)b->size[0];
  if (V.py < b->size[0]) FAIL(c, "%s: pitch_y %lld is below the block's %d voxels per row", who, b->pitch_y, b->size[0]);
  // (by division: py * size[1] <= pz exactly when py <= pz / size[1], and no product of a caller's numbers can overflow)
  if (V.py > LLONG_MAX / b->size[1] / b->size[2])
    FAIL(c, "%s: pitch_y %lld: a block of %d rows and %d slices of that pitch is beyond any address", who, b->pitch_y, b->size[1], b->size[2]);
  V.pz = b->pitch_z ? b->pitch_z : V.py * b->size[1];
  if (V.py > V.pz / b->size[1])
    FAIL(c, "%s: pitch_z %lld is below the block's %d rows of pitch %lld", who, b->pitch_z, b->size[1], V.py);
  if (V.pz > LLONG_MAX / b->size[2])
    FAIL(c, "%s: pitch_z %lld: a block of %d slices of that pitch is beyond any address", who, b->pitch_z, b->size[2]);
  for (int a = 0; a < 3; ++a)
    if (b->origin[a] < 0 || b->origin[a] > c->N[a] - b->size[a])
      FAIL(c, "%s: the block [%d, %d) of axis %c lies outside the volume %dx%dx%d (pass a view of the array that lies inside)", who, b->origin[a],
           b->origin[a] + b->size[a], "xyz"[a], c->N[0], c->N[1], c->N[2]);
  V.halo = c->halo;
  for (int a = 0; a < 3; ++a) {
    V.c0[a] = std::max(b->origin[a], c->O[a]);
    V.c1[a] = std::min(b->origin[a] + b->size[a], std::min(c->O[a] + c->D[a], c->N[a]));
    if (V.c0[a] > c->g0[a] || V.c1[a] < c->g1[a])
      FAIL(c, "%s: the block holds voxels [%d, %d) of axis %c inside this context's stored box, its region is [%d, %d): the block must contain "
              "the region", who, V.c0[a], std::max(V.c1[a], V.c0[a]), "xyz"[a], c->g0[a], c->g1[a]);
    // (beyond a face of C that is the volume's lies no voxel: that side gives all a halo can)
    if (c->g0[a] > 0 && V.c0[a] > 0) V.halo = std::min(V.halo, c->g0[a] - V.c0[a]);
    if (c->g1[a] < c->N[a] && V.c1[a] < c->N[a]) V.halo = std::min(V.halo, V.c1[a] - c->g1[a]);
  }
  return 0;
}

int smk_step_block_refusals(smk_ctx *c, const StencilEntry &E, int reach, const int *step_out, const smk_block *b, SmkBlockView &V) {
  const char *who = E.who;
  if (shard_context_refusals(c, E)) return 1;
  if (step_out && *step_out < 0) FAIL(c, "%s: time step %d: ids are >= 0", who, *step_out);
  if (smk_block_view(c, who, b, V)) return 1;
  if (c->nranks > 1 && V.halo < reach + 1)
    FAIL(c, "%s: the block gives a valid halo of %d voxels, the stencil reaches %d and the result keeps one for a frame: a valid halo >= %d is "
            "needed (ghost cells handed over, and option 'halo', set before the volume)", who, V.halo, reach, reach + 1);
  return 0;
}

void smk_step_block_box(const smk_ctx *c, const SmkBlockView &V, int reach, SmkShardBox &B) {
  for (int a = 0; a < 3; ++a) {
    B.O[a] = c->O[a];
    B.r0[a] = c->g0[a] - c->O[a];
    B.r1[a] = c->g1[a] - c->O[a];
    B.v0[a] = (V.c0[a] == 0 ? V.c0[a] : V.c0[a] + reach) - c->O[a];
    B.v1[a] = (V.c1[a] >= c->N[a] ? V.c1[a] : V.c1[a] - reach) - c->O[a];
  }
}

void smk_step_block_done(const smk_ctx *c, const SmkBlockView &V, int reach, const SmkShardBox &B, TimeStep &out) {
  out.valid_halo = c->nranks > 1 ? V.halo - reach : V.halo;
  for (int a = 0; a < 3; ++a) {
    out.vlo[a] = B.v0[a] + c->O[a];
    out.vhi[a] = B.v1[a] + c->O[a];
  }
}

extern "C" int smk_get_timestep_halo(smk_ctx *c, int timestep, int *valid_halo) {
  if (!c) return 1;
  const char *who = "smk_get_timestep_halo";
  int k = -1;
  if (step_slot(c, who, timestep, &k)) return 1;
  if (!valid_halo) FAIL(c, "%s: valid_halo is NULL", who);
  *valid_halo = c->ts[(size_t)k].valid_halo;
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
