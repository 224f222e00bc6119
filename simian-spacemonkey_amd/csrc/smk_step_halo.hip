// smk_step_halo.hip -- halo refill: a cached step's stored halo copied from the ranks that own those voxels (smk.h:
// smk_step_halo_layout, smk_step_halo_exports_device, smk_step_halo_entries_device, smk_step_halo_exchange_local; DESIGN.md
// 3b "Halo refill").
//
// The stencil producers on a shard move no voxel between ranks: their result is exact on the source's valid box less the
// reach, and the stored voxels beyond that are a rim of zeros.  Every voxel of that rim lies in exactly one other rank's
// region, where the same producer stored it exactly.  The refill moves those voxels: segment r->j is the box region_r ∩ S_j,
// S_j the box rank j stores cut at the volume.
//
// All the work is copies of sub-boxes between two arrays of packed voxels, and one kernel does all of them: a box of a slot
// into a packed segment (exports), a packed segment into a box of a slot (entries), a box of one slot into a box of another
// (the local exchange on one device).  A launch takes up to SMK_MAX_RANKS boxes by value.  Lanes run along x, then y, then z
// of a box and move 16 bytes each: one f32 voxel, or the two 8-byte voxels of a 16-byte unit OF THE DESTINATION -- a row whose
// first voxel is the high half of its unit starts with an 8-byte access, and so may its end; the source is then read as one
// 16-byte unit where it happens to be aligned alike and as two 8-byte voxels where not.  Plain loads and stores.
#include <algorithm>
#include <vector>

#include "smk_internal.h"

namespace {

constexpr unsigned HB_LANES = 256;

struct HaloBox {
  const void *src;            // the box's first voxel in the source array
  void *dst;                  // ... and in the destination array
  const uint32_t *src_n;      // its normal word in each (four-channel f32 with normals), or null
  uint32_t *dst_n;
  unsigned long long sp, ss;  // voxels between two rows and between two slices of the source
  unsigned long long dp, ds;  // ... of the destination
  unsigned long long units;   // upr * ny * nz
  unsigned first_block;       // workgroups of the boxes before this one
  unsigned nx, ny, upr;       // voxels per row, rows per slice, lanes per row
  StepDiv by_upr, by_ny;
};

struct HaloBoxes {
  HaloBox b[SMK_MAX_RANKS];
  int n;
};

typedef uint4 __attribute__((may_alias)) hb_u128;
typedef uint2 __attribute__((may_alias)) hb_u64;

// A workgroup belongs to one box (so the box's parameters stay in scalar registers); lane t of the box is unit t % upr of
// row t / upr.  WIDE: a unit is one 16-byte voxel and upr = nx.  Else a unit is an aligned pair of 8-byte voxels of the
// destination: with `head` = 1 where the row's first voxel is the high half of its unit, unit u holds the row's voxels
// 2u - head and 2u - head + 1, and upr = nx / 2 + 1 covers the row for either head
template <bool WIDE>
__global__ __launch_bounds__(256) void smk_k_halo_boxes(const HaloBoxes P) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < SMK_MAX_RANKS; ++i)
    if (i < P.n && blockIdx.x >= P.b[i].first_block) k = i;
  const HaloBox &B = P.b[k];
  const unsigned long long t = (unsigned long long)(blockIdx.x - B.first_block) * HB_LANES + threadIdx.x;
  if (t >= B.units) return;
  unsigned long long row, z;
  if (B.units <= 0xffffffffull) {
    row = step_divide((unsigned)t, B.by_upr);
    z = step_divide((unsigned)row, B.by_ny);
  } else {
    row = t / B.upr;
    z = row / B.ny;
  }
  const unsigned col = (unsigned)(t - row * B.upr);
  const unsigned long long y = row - z * B.ny;
  const unsigned long long so = z * B.ss + y * B.sp, dso = z * B.ds + y * B.dp;
  if (WIDE) {
    ((hb_u128 *)B.dst)[dso + col] = ((const hb_u128 *)B.src)[so + col];
    if (B.dst_n) B.dst_n[dso + col] = B.src_n[so + col];
  } else {
    const hb_u64 *src = (const hb_u64 *)B.src + so;
    hb_u64 *dst = (hb_u64 *)B.dst + dso;
    const unsigned head = (unsigned)(((uintptr_t)dst >> 3) & 1);
    const long long x = 2ll * col - head;  // the unit's low voxel in its row: -1 .. nx
    const bool lo = x >= 0 && x < (long long)B.nx, hi = x + 1 < (long long)B.nx;
    if (lo && hi) {
      uint4 v;
      if (((uintptr_t)(src + x) & 15) == 0) {
        v = *(const hb_u128 *)(src + x);
      } else {
        const uint2 a = src[x], b = src[x + 1];
        v = make_uint4(a.x, a.y, b.x, b.y);
      }
      *(hb_u128 *)(dst + x) = v;
    } else if (lo) {
      dst[x] = src[x];
    } else if (hi) {
      dst[x + 1] = src[x + 1];
    }
  }
}

// ---------------------------------------------------------------------------------------------- geometry (host)

inline long long roundup16(long long b) { return (b + 15) / 16 * 16; }

struct HaloSeg {
  int b0[3], b1[3];      // the box, global voxels; empty: nvox == 0
  long long nvox, bytes;  // voxels; bytes of the segment (voxels, then normal words)
  long long off;          // where it starts in the rank's exports / entries
};

struct HaloPlan {
  HaloSeg send[SMK_MAX_RANKS], recv[SMK_MAX_RANKS];  // segment rank->j; segment i->rank
  long long total_send = 0, total_recv = 0;
  long long VB = 8, NB = 0;
};

void halo_segment(const int g0[3], const int g1[3], const int s0[3], const int s1[3], long long VB, long long NB, HaloSeg &S) {
  S.nvox = 1;
  for (int a = 0; a < 3; ++a) {
    S.b0[a] = std::max(g0[a], s0[a]);
    S.b1[a] = std::min(g1[a], s1[a]);
    S.nvox *= std::max(S.b1[a] - S.b0[a], 0);
  }
  S.bytes = roundup16(S.nvox * VB) + roundup16(S.nvox * NB);
  S.off = 0;
}

// every rank's region and stored box cut at the volume, by this context's series and option "halo"; then this rank's segments
void halo_plan(const smk_ctx *c, HaloPlan &H) {
  H.VB = c->dtype == SMK_F32 ? 16 : 8;
  H.NB = smk_step_separate_normals(c) ? 4 : 0;
  int g0[SMK_MAX_RANKS][3], g1[SMK_MAX_RANKS][3], s0[SMK_MAX_RANKS][3], s1[SMK_MAX_RANKS][3];
  for (int j = 0; j < c->nranks; ++j) {
    int D[3];
    smk_shard_stored_box(c, j, g0[j], g1[j], s0[j], D);
    for (int a = 0; a < 3; ++a) s1[j][a] = std::min(s0[j][a] + D[a], c->N[a]);
  }
  const int r = c->rank;
  for (int j = 0; j < c->nranks; ++j) {
    halo_segment(g0[r], g1[r], s0[j], s1[j], H.VB, H.NB, H.send[j]);
    halo_segment(g0[j], g1[j], s0[r], s1[r], H.VB, H.NB, H.recv[j]);
    if (j == r) {
      H.send[j].nvox = H.send[j].bytes = 0;
      H.recv[j].nvox = H.recv[j].bytes = 0;
    }
    H.send[j].off = H.total_send;
    H.recv[j].off = H.total_recv;
    H.total_send += H.send[j].bytes;
    H.total_recv += H.recv[j].bytes;
  }
}

// ---------------------------------------------------------------------------------------------- boxes and launches (host)

// one side of a copy: an array of packed voxels with its pitches, and the voxel of it where global voxel `at` lies
struct HaloSide {
  char *vox, *nrm;              // the arrays' first voxel and normal word (nrm null: none)
  unsigned long long p, s;      // voxels between rows, between slices
  int at[3];                    // the global voxel of element 0
};

HaloSide slot_side(const smk_ctx *c, const TimeStep &T) {
  HaloSide S;
  S.vox = (char *)T.vox;
  S.nrm = smk_step_separate_normals(c) ? (char *)T.nrm : nullptr;
  S.p = (unsigned long long)c->D[0];
  S.s = (unsigned long long)c->D[0] * c->D[1];
  for (int a = 0; a < 3; ++a) S.at[a] = c->O[a];
  return S;
}

// a packed segment in a caller's buffer: the box itself, dense
HaloSide segment_side(const HaloPlan &H, const HaloSeg &G, const void *buf) {
  HaloSide S;
  S.vox = (char *)buf + G.off;
  S.nrm = H.NB ? S.vox + roundup16(G.nvox * H.VB) : nullptr;
  S.p = (unsigned long long)(G.b1[0] - G.b0[0]);
  S.s = S.p * (unsigned long long)(G.b1[1] - G.b0[1]);
  for (int a = 0; a < 3; ++a) S.at[a] = G.b0[a];
  return S;
}

void add_box(HaloBoxes &L, unsigned &blocks, const HaloPlan &H, const HaloSeg &G, const HaloSide &src, const HaloSide &dst) {
  if (!G.nvox) return;
  HaloBox &B = L.b[L.n++];
  const auto first = [&](const HaloSide &S) {
    return ((unsigned long long)(G.b0[2] - S.at[2]) * S.s + (unsigned long long)(G.b0[1] - S.at[1]) * S.p + (unsigned long long)(G.b0[0] - S.at[0]));
  };
  const unsigned long long fs = first(src), fd = first(dst);
  B.src = src.vox + fs * H.VB;
  B.dst = dst.vox + fd * H.VB;
  B.src_n = src.nrm && dst.nrm ? (const uint32_t *)(src.nrm + fs * 4) : nullptr;
  B.dst_n = src.nrm && dst.nrm ? (uint32_t *)(dst.nrm + fd * 4) : nullptr;
  B.sp = src.p;
  B.ss = src.s;
  B.dp = dst.p;
  B.ds = dst.s;
  B.nx = (unsigned)(G.b1[0] - G.b0[0]);
  B.ny = (unsigned)(G.b1[1] - G.b0[1]);
  B.upr = H.VB == 16 ? B.nx : B.nx / 2 + 1;
  B.units = (unsigned long long)B.upr * B.ny * (unsigned long long)(G.b1[2] - G.b0[2]);
  B.by_upr = step_div(B.upr);
  B.by_ny = step_div(B.ny);
  B.first_block = blocks;
  blocks += (unsigned)((B.units + HB_LANES - 1) / HB_LANES);
}

hipError_t launch_boxes(const HaloBoxes &L, unsigned blocks, bool wide, hipStream_t s) {
  if (!L.n) return hipSuccess;
  if (wide) hipLaunchKernelGGL(smk_k_halo_boxes<true>, dim3(blocks), dim3(HB_LANES), 0, s, L);
  else hipLaunchKernelGGL(smk_k_halo_boxes<false>, dim3(blocks), dim3(HB_LANES), 0, s, L);
  return hipGetLastError();
}

// what a refilled step has valid: the stored box cut at the volume, and all of option "halo"
void whole_again(const smk_ctx *c, TimeStep &T) {
  T.valid_halo = c->halo;
  for (int a = 0; a < 3; ++a) {
    T.vlo[a] = c->O[a];
    T.vhi[a] = std::min(c->O[a] + c->D[a], c->N[a]);
  }
}

int buffer_refusals(smk_ctx *c, const char *who, const char *name, const void *p, long long bytes) {
  if (!bytes) return 0;
  if (!p) FAIL(c, "%s: %s is NULL and %lld bytes are due (smk_step_halo_layout)", who, name, bytes);
  if ((uintptr_t)p % 16) FAIL(c, "%s: %s is not aligned to 16 bytes", who, name);
  return 0;
}

int exports_enqueue(smk_ctx *c, const HaloPlan &H, int k, void *d_exports, hipStream_t s) {
  return smk_step_read(c, k, -1, s, [&]() -> int {
    HaloBoxes L;
    L.n = 0;
    unsigned blocks = 0;
    const HaloSide slot = slot_side(c, c->ts[(size_t)k]);
    for (int j = 0; j < c->nranks; ++j) add_box(L, blocks, H, H.send[j], slot, segment_side(H, H.send[j], d_exports));
    HIPCHK(c, launch_boxes(L, blocks, H.VB == 16, s));
    return 0;
  });
}

int entries_enqueue(smk_ctx *c, const HaloPlan &H, int k, const void *d_entries, hipStream_t s) {
  return smk_step_rewrite(c, k, s, [&](TimeStep &T) -> int {
    HaloBoxes L;
    L.n = 0;
    unsigned blocks = 0;
    const HaloSide slot = slot_side(c, T);
    for (int i = 0; i < c->nranks; ++i) add_box(L, blocks, H, H.recv[i], segment_side(H, H.recv[i], d_entries), slot);
    HIPCHK(c, launch_boxes(L, blocks, H.VB == 16, s));
    whole_again(c, T);
    return 0;
  });
}

// the refusals the entries share; *k: the step's slot
int entry_refusals(smk_ctx *c, const char *who, int timestep, int *k) {
  HIPCHK(c, hipSetDevice(c->device));
  return step_slot(c, who, timestep, k);
}

// the local exchange on one device: receiver j's halo straight from the owners' slots, as a reader of every owner (each
// bracket inside the one before it) and a writer of j, on stream s
int direct_reads(smk_ctx *const *all, const std::vector<int> &ks, int j, int i, hipStream_t s, const std::function<int()> &launch) {
  smk_ctx *cj = all[j];
  if (i == cj->nranks) return launch();
  if (i == j) return direct_reads(all, ks, j, i + 1, s, launch);
  return smk_step_read(all[i], ks[(size_t)i], -1, s, [&]() -> int { return direct_reads(all, ks, j, i + 1, s, launch); });
}

int direct_enqueue(smk_ctx *const *all, const std::vector<int> &ks, int j, hipStream_t s) {
  smk_ctx *c = all[j];
  HaloPlan H;
  halo_plan(c, H);
  return smk_step_rewrite(c, ks[(size_t)j], s, [&](TimeStep &T) -> int {
    return direct_reads(all, ks, j, 0, s, [&]() -> int {
      HaloBoxes L;
      L.n = 0;
      unsigned blocks = 0;
      const HaloSide slot = slot_side(c, T);
      for (int i = 0; i < c->nranks; ++i)
        if (i != j) add_box(L, blocks, H, H.recv[i], slot_side(all[i], all[i]->ts[(size_t)ks[(size_t)i]]), slot);
      HIPCHK(c, launch_boxes(L, blocks, H.VB == 16, s));
      whole_again(c, T);
      return 0;
    });
  });
}

int stage_reserve(smk_ctx *c, int which, long long bytes) {
  if ((size_t)bytes <= c->halo_stage_cap[which]) return 0;
  if (c->d_halo_stage[which]) (void)hipFree(c->d_halo_stage[which]);
  c->d_halo_stage[which] = nullptr;
  c->halo_stage_cap[which] = 0;
  HIPCHK(c, hipMalloc(&c->d_halo_stage[which], (size_t)bytes));
  c->halo_stage_cap[which] = (size_t)bytes;
  return 0;
}

}  // namespace

extern "C" int smk_step_halo_layout(smk_ctx *c, long long *send_bytes, long long *recv_bytes, long long *total_send, long long *total_recv) {
  if (!c) return 1;
  if (!c->have_volume) FAIL(c, "smk_step_halo_layout: no volume uploaded (smk_declare_volume gives a context its geometry without data)");
  HaloPlan H;
  halo_plan(c, H);
  for (int j = 0; j < c->nranks; ++j) {
    if (send_bytes) send_bytes[j] = H.send[j].bytes;
    if (recv_bytes) recv_bytes[j] = H.recv[j].bytes;
  }
  if (total_send) *total_send = H.total_send;
  if (total_recv) *total_recv = H.total_recv;
  return 0;
}

extern "C" int smk_step_halo_exports_device(smk_ctx *c, int timestep, void *d_exports, void *stream) {
  if (!c) return 1;
  const char *who = "smk_step_halo_exports_device";
  int k = -1;
  if (entry_refusals(c, who, timestep, &k)) return 1;
  if (c->nranks == 1) return 0;
  HaloPlan H;
  halo_plan(c, H);
  if (buffer_refusals(c, who, "d_exports", d_exports, H.total_send)) return 1;
  return exports_enqueue(c, H, k, d_exports, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_step_halo_entries_device(smk_ctx *c, int timestep, const void *d_entries, void *stream) {
  if (!c) return 1;
  const char *who = "smk_step_halo_entries_device";
  int k = -1;
  if (entry_refusals(c, who, timestep, &k)) return 1;
  if (c->nranks == 1) return 0;
  HaloPlan H;
  halo_plan(c, H);
  if (buffer_refusals(c, who, "d_entries", d_entries, H.total_recv)) return 1;
  return entries_enqueue(c, H, k, d_entries, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_step_halo_exchange_local(smk_ctx *const *all, int nranks, int timestep, void *stream) {
  const char *who = "smk_step_halo_exchange_local";
  if (!all || nranks < 1 || nranks > SMK_MAX_RANKS) return 1;
  for (int r = 0; r < nranks; ++r)
    if (!all[r]) return 1;
  for (int r = 0; r < nranks; ++r) all[r]->err.clear();  // (after a failure the one message left is this call's, on the context it concerns)
  // every refusal before anything is enqueued: a refused call changes nothing
  std::vector<int> ks((size_t)nranks, -1);
  bool one_device = true;
  for (int r = 0; r < nranks; ++r) {
    smk_ctx *c = all[r];
    if (c->nranks != nranks || c->rank != r) FAIL(c, "%s: context %d is not shard %d of %d (it is shard %d of %d)", who, r, r, nranks, c->rank, c->nranks);
    if (entry_refusals(c, who, timestep, &ks[(size_t)r])) return 1;
    const smk_ctx *z = all[0];
    for (int a = 0; a < 3; ++a)
      if (c->N[a] != z->N[a])
        FAIL(c, "%s: rank %d differs from rank 0 in dims: %dx%dx%d, not %dx%dx%d", who, r, c->N[0], c->N[1], c->N[2], z->N[0], z->N[1], z->N[2]);
    if (c->dtype != z->dtype) FAIL(c, "%s: rank %d differs from rank 0 in dtype: %d, not %d", who, r, c->dtype, z->dtype);
    if (c->nelts != z->nelts) FAIL(c, "%s: rank %d differs from rank 0 in nelts: %d, not %d", who, r, c->nelts, z->nelts);
    if (c->have_normals != z->have_normals)
      FAIL(c, "%s: rank %d differs from rank 0 in normals: %s, not %s", who, r, c->have_normals ? "present" : "absent", z->have_normals ? "present" : "absent");
    if (c->halo != z->halo) FAIL(c, "%s: rank %d differs from rank 0 in halo: %d, not %d", who, r, c->halo, z->halo);
    one_device = one_device && c->device == z->device;
  }
  if (nranks == 1) return 0;
  if (stream && !one_device)
    FAIL(all[0], "%s: a caller's stream serves one device and the contexts lie on several: pass stream NULL", who);
  const auto sync_all = [&]() -> int {
    for (int r = 0; r < nranks; ++r) {
      HIPCHK(all[r], hipSetDevice(all[r]->device));
      HIPCHK(all[r], hipStreamSynchronize(all[r]->stream));
    }
    return 0;
  };
  if (one_device) {
    for (int j = 0; j < nranks; ++j)
      if (direct_enqueue(all, ks, j, stream ? (hipStream_t)stream : all[j]->stream)) return 1;
    return stream ? 0 : sync_all();
  }
  // several devices: every rank's exports into its staging buffer, peer copies of the segments, every rank's entries
  std::vector<HaloPlan> H((size_t)nranks);
  for (int r = 0; r < nranks; ++r) {
    smk_ctx *c = all[r];
    HIPCHK(c, hipSetDevice(c->device));
    halo_plan(c, H[(size_t)r]);
    if (stage_reserve(c, 0, H[(size_t)r].total_send) || stage_reserve(c, 1, H[(size_t)r].total_recv)) return 1;
  }
  if (sync_all()) return 1;  // (the staging buffers' last readers are done)
  for (int r = 0; r < nranks; ++r) {
    HIPCHK(all[r], hipSetDevice(all[r]->device));
    if (exports_enqueue(all[r], H[(size_t)r], ks[(size_t)r], all[r]->d_halo_stage[0], all[r]->stream)) return 1;
  }
  for (int r = 0; r < nranks; ++r) {
    smk_ctx *c = all[r];
    HIPCHK(c, hipSetDevice(c->device));
    for (int j = 0; j < nranks; ++j) {
      const HaloSeg &G = H[(size_t)r].send[j];
      if (!G.bytes) continue;
      char *to = (char *)all[j]->d_halo_stage[1] + H[(size_t)j].recv[r].off;
      const char *from = (const char *)c->d_halo_stage[0] + G.off;
      if (all[j]->device == c->device) HIPCHK(c, hipMemcpyAsync(to, from, (size_t)G.bytes, hipMemcpyDeviceToDevice, c->stream));
      else HIPCHK(c, hipMemcpyPeerAsync(to, all[j]->device, from, c->device, (size_t)G.bytes, c->stream));
    }
  }
  if (sync_all()) return 1;
  for (int j = 0; j < nranks; ++j) {
    HIPCHK(all[j], hipSetDevice(all[j]->device));
    if (entries_enqueue(all[j], H[(size_t)j], ks[(size_t)j], all[j]->d_halo_stage[1], all[j]->stream)) return 1;
  }
  return sync_all();
}
