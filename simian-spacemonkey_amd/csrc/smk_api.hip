// smk_api.hip -- the C ABI (include/smk.h): context, HBM layout, host-side setup, statistics, slice quads and the sort-last
// merge.  A frame is smk_frame.hip's; the host side of shadows is smk_shadow_plan.hip's.
// Product code: no CPU rendering path exists here; without a HIP device every entry fails.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "smk_device.h"

static std::string g_create_err;

// ------------------------------------------------------------------------------- host thread pool
// Planning a frame (the slice-ring launcher's scan of every tile's ray bundle) is double arithmetic on the host's thread:
// a pool of a few workers shares it.  One pool per process; contexts are used from one thread at a time (smk.h), a mutex
// keeps two contexts on different threads from interleaving jobs.
#include <condition_variable>
#include <mutex>
#include <thread>
namespace {
struct HostPool {
  std::vector<std::thread> workers;
  std::mutex m, use;
  std::condition_variable cv, done_cv;
  const std::function<void(int)> *job = nullptr;
  int njobs = 0, next = 0, pending = 0;
  unsigned long long gen = 0;
  bool quit = false;
  explicit HostPool(int n) {
    for (int i = 0; i < n; ++i)
      workers.emplace_back([this] {
        unsigned long long seen = 0;
        for (;;) {
          std::unique_lock<std::mutex> lk(m);
          cv.wait(lk, [&] { return quit || (gen != seen && next < njobs); });
          if (quit) return;
          while (next < njobs) {
            const int k = next++;
            lk.unlock();
            (*job)(k);
            lk.lock();
            if (--pending == 0) done_cv.notify_all();
          }
          seen = gen;
        }
      });
  }
  ~HostPool() {
    {
      std::lock_guard<std::mutex> lk(m);
      quit = true;
    }
    cv.notify_all();
    for (std::thread &t : workers) t.join();
  }
};
HostPool *host_pool() {
  static HostPool *pool = [] {
    const char *e = getenv("SMK_HOST_THREADS");
    int n = e ? atoi(e) : (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency() / 2));
    n = std::max(1, std::min(n, 32));
    return new HostPool(n - 1);  // (the caller is the n-th; never destroyed: workers must not outlive a static's destructor order)
  }();
  return pool;
}
}  // namespace

int smk_host_pool_size() { return (int)host_pool()->workers.size() + 1; }

void smk_host_pool_run(int n, const std::function<void(int)> &f) {
  HostPool *p = host_pool();
  if (n <= 1 || p->workers.empty()) {
    for (int k = 0; k < n; ++k) f(k);
    return;
  }
  std::lock_guard<std::mutex> one(p->use);
  {
    std::lock_guard<std::mutex> lk(p->m);
    p->job = &f;
    p->njobs = n;
    p->next = 1;        // job 0 is the caller's
    p->pending = n - 1;
    ++p->gen;
  }
  p->cv.notify_all();
  f(0);
  std::unique_lock<std::mutex> lk(p->m);
  // (help with what is left rather than wait for a worker to wake up)
  while (p->next < p->njobs) {
    const int k = p->next++;
    lk.unlock();
    f(k);
    lk.lock();
    --p->pending;
  }
  p->done_cv.wait(lk, [&] { return p->pending == 0; });
  p->job = nullptr;
  p->njobs = 0;
}

// ------------------------------------------------------------------------------- lifecycle

extern "C" smk_ctx *smk_create(int device_ordinal, int *err) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_err = "smk_create: no HIP device available (this library has no CPU fallback)";
    if (err) *err = 1;
    return nullptr;
  }
  if (device_ordinal < 0 || device_ordinal >= n) {
    g_create_err = "smk_create: device ordinal out of range";
    if (err) *err = 2;
    return nullptr;
  }
  if (hipSetDevice(device_ordinal) != hipSuccess) {
    g_create_err = "smk_create: hipSetDevice failed";
    if (err) *err = 3;
    return nullptr;
  }
  smk_ctx *c = new smk_ctx();
  c->device = device_ordinal;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    g_create_err = "smk_create: stream/event creation failed";
    delete c;
    if (err) *err = 4;
    return nullptr;
  }
  if (err) *err = 0;
  return c;
}

static void free_brick_set(BrickSet &B) {
  if (B.flags) (void)hipFree(B.flags);
  if (B.dil) (void)hipFree(B.dil);
  if (B.sat) (void)hipFree(B.sat);
  if (B.d_count) (void)hipFree(B.d_count);
  if (B.h_count) (void)hipHostFree(B.h_count);
  if (B.counted) (void)hipEventDestroy(B.counted);
  B = BrickSet();
}

static void free_volume(smk_ctx *c) {
  smk_free_steps(c);  // (every cached step: the current one's d_vox, d_nrm, d_vox_x, d_brick_mm among them)
  smk_cols_drop_layouts(&c->cols);  // (built from this volume)
  c->d_brick_mm = nullptr;
  c->d_vox_x = nullptr;
  c->d_vox = nullptr;
  c->d_nrm = nullptr;
  c->have_volume = false;
}

extern "C" void smk_destroy(smk_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  free_volume(c);
  for (smk_ctx::TfVersion &T : c->tfv) {
    if (T.d) (void)hipFree(T.d);
    if (T.h) (void)hipHostFree(T.h);
    free_brick_set(T.br);
    if (T.copied) (void)hipEventDestroy(T.copied);
    if (T.used) (void)hipEventDestroy(T.used);
  }
  if (c->tf_raw_ev) (void)hipEventDestroy(c->tf_raw_ev);
  if (c->tf_ready) (void)hipEventDestroy(c->tf_ready);
  if (c->tf_stream) { (void)hipStreamSynchronize(c->tf_stream); (void)hipStreamDestroy(c->tf_stream); }
  free_brick_set(c->br3);
  smk_cols_free(&c->cols);
  smk_present_free(c);  // (the slots' device and pinned buffers, the copy stream)
  void *ptrs[] = {c->d_light_hist, c->d_shadow_entries, c->d_shadow_exports, c->d_halo_stage[0], c->d_halo_stage[1], c->d_shadow_barrier, c->d_tf_raw, c->d_tlut, c->d_tf_h, c->d_tf3d, c->d_tf3d_occ, c->d_noise, c->d_out, c->d_depth, c->d_zscene, c->d_light[0], c->d_light[1]};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  smk_slab_free(&c->slab);
  for (hipEvent_t e : c->tev0) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->tev1) (void)hipEventDestroy(e);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" const char *smk_last_error(smk_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

// ------------------------------------------------------------------------------- volume upload

// source voxel (brick-local, caller layout [z][y][x][nelts] + optional [z][y][x][3] normals)
// -> packed voxel in the dense region+halo box.  One thread per source voxel of the chunk.
template <int DT>
__global__ void smk_k_pack(const void *src, const unsigned char *grad, int bx, int by, int cz, int nelts,
                           int gx0, int gy0, int gz0,  // global index of the chunk's first voxel
                           int Ox, int Oy, int Oz, int Dx, int Dy, int Dz, void *dst, uint32_t *nrm, int n_in_w) {
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t total = (size_t)bx * by * cz;
  if (t >= total) return;
  int x = (int)(t % bx);
  int y = (int)((t / bx) % by);
  int z = (int)(t / ((size_t)bx * by));
  int X = gx0 + x - Ox, Y = gy0 + y - Oy, Z = gz0 + z - Oz;
  if (X < 0 || X >= Dx || Y < 0 || Y >= Dy || Z < 0 || Z >= Dz) return;
  size_t o = ((size_t)Z * Dy + Y) * Dx + X;
  uint32_t nb = SMK_NRM_NONE;
  if (grad) nb = smk_nrm_word(grad[t * 3], grad[t * 3 + 1], grad[t * 3 + 2]);
  if (DT == SMK_U8) {
    ((uint2 *)dst)[o] = smk_pack_u8((const unsigned char *)src + t * nelts, nelts, nb);
  } else if (DT == SMK_U16) {
    ((uint2 *)dst)[o] = smk_pack_u16((const unsigned short *)src + t * nelts, nelts, nb);
  } else {
    const uint4 v = smk_pack_f32((const float *)src + t * nelts, nelts, nb, n_in_w);
    if (!n_in_w && nrm) nrm[o] = nb;
    ((uint4 *)dst)[o] = v;
  }
}

// the region of shard `rank` of `nranks` of an N[0] x N[1] x N[2] volume
static void shard_box(const int N[3], int rank, int nranks, int g0[3], int g1[3]) {
  for (int a = 0; a < 3; ++a) {
    g0[a] = 0;
    g1[a] = N[a];
  }
  int bit = 0;
  for (int n = nranks; n > 1; n >>= 1, ++bit) {
    int a = bit % 3, half = N[a] / 2;  // bit 0 splits x, bit 1 y, bit 2 z
    if ((rank >> bit) & 1) g0[a] = std::max(g0[a], half);
    else g1[a] = std::min(g1[a], half);
  }
}

void smk_shard_region(const smk_ctx *c, int rank, int g0[3], int g1[3]) { shard_box(c->N, rank, c->nranks, g0, g1); }

// the region of shard `rank` and the box it stores: the region plus `halo` voxels, cut at the volume; true when the box has a
// pad column or row.
// 8-byte voxels travel to LDS in 16-byte units: the slice-ring kernel wants even row lengths
// along both axes that can be its contiguous one (x, and y in the x-major copy) -- one more halo
// voxel where the volume has one, else a pad column nobody samples (index N: the texel pair of a
// clamped coordinate ends at N-1)
static bool stored_box(const int N[3], int dtype, int halo, int rank, int nranks, int g0[3], int g1[3], int O[3], int D[3]) {
  bool padded = false;
  shard_box(N, rank, nranks, g0, g1);
  for (int a = 0; a < 3; ++a) {
    int lo = std::max(g0[a] - halo, 0), hi = std::min(g1[a] + halo, N[a]);
    O[a] = lo;
    D[a] = hi - lo;
  }
  if (dtype != SMK_F32)
    for (int a = 0; a < 2; ++a)
      if (D[a] & 1) {
        if (O[a] + D[a] < N[a]) ++D[a];
        else if (O[a] > 0) { --O[a]; ++D[a]; }
        else { ++D[a]; padded = true; }
      }
  return padded;
}

void smk_shard_stored_box(const smk_ctx *c, int rank, int g0[3], int g1[3], int O[3], int D[3]) {
  (void)stored_box(c->N, c->dtype, c->halo, rank, c->nranks, g0, g1, O, D);
}

// whole-volume dims and extent from the brick list (MetaVolume::brick keeps iPos/fPos), and the box this context stores
int smk_volume_geometry(smk_ctx *c, const char *who, const smk_volume_desc *b, int nb, int nelts, smk_dtype dtype,
                        smk_datamode dmode, SmkVolGeom &g) {
  if (!b || nb <= 0) FAIL(c, "%s: no bricks", who);
  if (nelts < 1 || nelts > 4) FAIL(c, "%s: nelts %d not in 1..4", who, nelts);
  if (dtype != SMK_U8 && dtype != SMK_F32 && dtype != SMK_U16) FAIL(c, "%s: bad dtype", who);
  if (dtype == SMK_U16 && nelts == 4)
    FAIL(c, "%s: 4-channel u16 voxels do not fit the 8-byte packed voxel (nelts 1..3; smk.h SMK_U16)", who);
  g = SmkVolGeom();
  g.dtype = dtype;
  g.nelts = nelts;
  g.dmode = dmode;
  int *N = g.N;
  float *fs = g.fs;
  bool any_grad = false, all_grad = true;
  for (int i = 0; i < nb; ++i) {
    if (!b[i].data) FAIL(c, "%s: brick %d has no data", who, i);
    if (b[i].xiSize <= 0 || b[i].yiSize <= 0 || b[i].ziSize <= 0) FAIL(c, "%s: brick %d empty", who, i);
    if (b[i].xiPos < 0 || b[i].yiPos < 0 || b[i].ziPos < 0) FAIL(c, "%s: brick %d negative origin", who, i);
    N[0] = std::max(N[0], b[i].xiPos + b[i].xiSize);
    N[1] = std::max(N[1], b[i].yiPos + b[i].yiSize);
    N[2] = std::max(N[2], b[i].ziPos + b[i].ziSize);
    fs[0] = std::max(fs[0], b[i].xfPos + b[i].xfSize);
    fs[1] = std::max(fs[1], b[i].yfPos + b[i].yfSize);
    fs[2] = std::max(fs[2], b[i].zfPos + b[i].zfSize);
    any_grad |= b[i].grad != nullptr;
    all_grad &= b[i].grad != nullptr;
  }
  if (any_grad && !all_grad) FAIL(c, "%s: some bricks have normals and some do not", who);
  size_t vox = 0;
  for (int i = 0; i < nb; ++i) vox += (size_t)b[i].xiSize * b[i].yiSize * b[i].ziSize;
  if (vox != (size_t)N[0] * N[1] * N[2]) FAIL(c, "%s: bricks do not tile the %dx%dx%d volume", who, N[0], N[1], N[2]);
  if (!(fs[0] > 0 && fs[1] > 0 && fs[2] > 0)) FAIL(c, "%s: non-positive extent", who);
  if (c->nranks > 1)
    for (int a = 0; a < 3; ++a)
      if (N[a] < 2) FAIL(c, "%s: volume too thin to shard", who);
  g.grad = any_grad;
  g.padded = stored_box(N, dtype, c->halo, c->rank, c->nranks, g.g0, g.g1, g.O, g.D);
  const size_t nst = (size_t)g.D[0] * g.D[1] * g.D[2];
  g.vox_bytes = nst * (dtype == SMK_F32 ? 16 : 8);
  g.nrm_bytes = dtype == SMK_F32 && nelts == 4 && any_grad ? nst * 4 : 0;
  for (int a = 0; a < 3; ++a) g.nbr[a] = (g.D[a] - 1) / (1 << SMK_BRICK_LOG2) + 1;
  g.mm_bytes = (size_t)g.nbr[0] * g.nbr[1] * g.nbr[2] * sizeof(float4);
  return 0;
}

// the context's volume geometry becomes g's (the first upload of a volume or a series)
void smk_set_geometry(smk_ctx *c, const SmkVolGeom &g) {
  c->dtype = g.dtype;
  c->nelts = g.nelts;
  c->dmode = g.dmode;
  for (int a = 0; a < 3; ++a) {
    c->N[a] = g.N[a];
    c->fsize[a] = g.fs[a];
    c->g0[a] = g.g0[a];
    c->g1[a] = g.g1[a];
    c->O[a] = g.O[a];
    c->D[a] = g.D[a];
    c->nbr[a] = g.nbr[a];
  }
  c->vox_bytes = g.vox_bytes;
  c->have_normals = g.grad;
}

int smk_alloc_step(smk_ctx *c, const SmkVolGeom &g, TimeStep &T) {
  if (!T.vox) {
    HIPCHK(c, hipMalloc(&T.vox, g.vox_bytes + 16));  // (+16: the gather kernel reads 8-byte voxels in pairs, smk_load_pair_u8 / _u16)
    if (g.padded) HIPCHK(c, hipMemset(T.vox, 0, g.vox_bytes));
  }
  if (g.nrm_bytes && !T.nrm) HIPCHK(c, hipMalloc((void **)&T.nrm, g.nrm_bytes));
  if (!T.mm) HIPCHK(c, hipMalloc((void **)&T.mm, g.mm_bytes));
  if (!T.pass1_words) HIPCHK(c, hipMalloc((void **)&T.pass1_words, 8 * sizeof(int)));  // (with the slot: a producer allocates nothing)
  return 0;
}

// Packs the bricks into step T's buffers and makes its brick summaries.  s == null: synchronous, host bricks staged in chunks
// (smk_upload_volume); else everything is enqueued on s, which must then also order the reads of the caller's (device)
// bricks.  The pad column of a padded box was cleared when the buffer was made, and no brick writes it.
int smk_pack_step(smk_ctx *c, const char *who, const SmkVolGeom &g, const smk_volume_desc *b, int nb, bool on_device, TimeStep &T,
                  hipStream_t s) {
  const int nelts = g.nelts;
  const size_t esz = g.dtype == SMK_U8 ? 1 : g.dtype == SMK_U16 ? 2 : 4;
  const bool n_in_w = g.dtype == SMK_F32 && nelts <= 3;
  void *d_stage = nullptr;
  unsigned char *d_gstage = nullptr;
  const size_t chunk_budget = (size_t)256 << 20;
  for (int i = 0; i < nb; ++i) {
    const smk_volume_desc &k = b[i];
    // skip bricks that cannot touch this context's stored box
    if (k.xiPos >= g.O[0] + g.D[0] || k.xiPos + k.xiSize <= g.O[0] || k.yiPos >= g.O[1] + g.D[1] ||
        k.yiPos + k.yiSize <= g.O[1] || k.ziPos >= g.O[2] + g.D[2] || k.ziPos + k.ziSize <= g.O[2])
      continue;
    size_t slice = (size_t)k.xiSize * k.yiSize;
    int zper = on_device ? k.ziSize : (int)std::max<size_t>(1, chunk_budget / (slice * nelts * esz));
    for (int z0 = 0; z0 < k.ziSize; z0 += zper) {
      int cz = std::min(zper, k.ziSize - z0);
      // only the z range that intersects the stored box
      if (k.ziPos + z0 >= g.O[2] + g.D[2] || k.ziPos + z0 + cz <= g.O[2]) continue;
      const void *src;
      const unsigned char *gsrc = nullptr;
      size_t off = (size_t)z0 * slice;
      if (on_device) {
        src = (const char *)k.data + off * nelts * esz;
        if (k.grad) gsrc = k.grad + off * 3;
      } else {
        if (!d_stage) HIPCHK(c, hipMalloc(&d_stage, std::min(chunk_budget + slice * nelts * esz, (size_t)-1)));
        size_t bytes = (size_t)cz * slice * nelts * esz;
        if (bytes > chunk_budget + slice * nelts * esz) FAIL(c, "%s: internal staging overflow", who);
        HIPCHK(c, hipMemcpy(d_stage, (const char *)k.data + off * nelts * esz, bytes, hipMemcpyHostToDevice));
        src = d_stage;
        if (k.grad) {
          if (!d_gstage) HIPCHK(c, hipMalloc((void **)&d_gstage, ((size_t)zper + 1) * slice * 3));
          HIPCHK(c, hipMemcpy(d_gstage, k.grad + off * 3, (size_t)cz * slice * 3, hipMemcpyHostToDevice));
          gsrc = d_gstage;
        }
      }
      size_t total = (size_t)cz * slice;
      unsigned blocks = (unsigned)((total + 255) / 256);
      if (g.dtype == SMK_U8)
        hipLaunchKernelGGL(smk_k_pack<0>, dim3(blocks), dim3(256), 0, s, src, gsrc, k.xiSize, k.yiSize, cz, nelts,
                           k.xiPos, k.yiPos, k.ziPos + z0, g.O[0], g.O[1], g.O[2], g.D[0], g.D[1], g.D[2],
                           T.vox, T.nrm, 0);
      else if (g.dtype == SMK_U16)
        hipLaunchKernelGGL(smk_k_pack<2>, dim3(blocks), dim3(256), 0, s, src, gsrc, k.xiSize, k.yiSize, cz, nelts,
                           k.xiPos, k.yiPos, k.ziPos + z0, g.O[0], g.O[1], g.O[2], g.D[0], g.D[1], g.D[2],
                           T.vox, T.nrm, 0);
      else
        hipLaunchKernelGGL(smk_k_pack<1>, dim3(blocks), dim3(256), 0, s, src, gsrc, k.xiSize, k.yiSize, cz, nelts,
                           k.xiPos, k.yiPos, k.ziPos + z0, g.O[0], g.O[1], g.O[2], g.D[0], g.D[1], g.D[2],
                           T.vox, T.nrm, n_in_w ? 1 : 0);
      HIPCHK(c, hipGetLastError());
      if (!s) HIPCHK(c, hipDeviceSynchronize());
    }
  }
  if (d_stage) (void)hipFree(d_stage);
  if (d_gstage) (void)hipFree(d_gstage);
  // value ranges of the 8x8x8-cell bricks (smk_bricks.hip): what the brick flags of every later table are made from
  HIPCHK(c, smk_bricks_minmax(T.vox, g.dtype, g.D, g.nbr, T.mm, s));
  if (!s) HIPCHK(c, hipDeviceSynchronize());
  T.vox_x_valid = false;
  // an upload fills the stored box: all of it that lies in the volume is valid
  T.valid_halo = c->halo;
  for (int a = 0; a < 3; ++a) {
    T.vlo[a] = g.O[a];
    T.vhi[a] = std::min(g.O[a] + g.D[a], g.N[a]);
  }
  return 0;
}

static int upload_impl(smk_ctx *c, const smk_volume_desc *b, int nb, int nelts, smk_dtype dtype, smk_datamode dmode,
                       bool on_device) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  SmkVolGeom g;
  if (smk_volume_geometry(c, "smk_upload_volume", b, nb, nelts, dtype, dmode, g)) return 1;
  // every cached time step goes; the volume is stored as the current step
  free_volume(c);
  smk_set_geometry(c, g);
  c->ts.assign((size_t)c->ts_cap, TimeStep());
  TimeStep &T = c->ts[0];
  if (smk_alloc_step(c, g, T)) return 1;
  T.id = c->ts_cur_id;
  T.written = ++c->ts_written;
  if (smk_pack_step(c, "smk_upload_volume", g, b, nb, on_device, T, nullptr)) return 1;
  smk_use_step(c, 0);
  c->tune_choice.clear();  // a new volume: the kernels' relative speed is measured afresh
  c->tune_sig = 0;
  return 0;
}

extern "C" int smk_upload_volume(smk_ctx *c, const smk_volume_desc *b, int nb, int nelts, smk_dtype dt,
                                 smk_datamode dm) {
  return upload_impl(c, b, nb, nelts, dt, dm, false);
}
extern "C" int smk_upload_volume_device(smk_ctx *c, const smk_volume_desc *b, int nb, int nelts, smk_dtype dt,
                                        smk_datamode dm) {
  return upload_impl(c, b, nb, nelts, dt, dm, true);
}

// The geometry of a series without data (smk.h): upload_impl for a volume of zeros that nobody holds.  The geometry and its
// refusals are smk_volume_geometry's own, asked about ONE brick that is the whole volume; its data pointer only has to be
// non-null there, and nothing reads it: smk_pack_block without a source fills the stored box
extern "C" int smk_declare_volume(smk_ctx *c, const int dims[3], const float extent[3], int nelts, smk_dtype dtype, smk_datamode dmode,
                                  int normals) {
  if (!c) return 1;
  const char *who = "smk_declare_volume";
  HIPCHK(c, hipSetDevice(c->device));
  if (!dims || !extent) FAIL(c, "%s: dims or extent is NULL", who);
  static const unsigned char nobody = 0;
  smk_volume_desc b = {dims[0], dims[1], dims[2], extent[0], extent[1], extent[2], 0, 0, 0, 0.f, 0.f, 0.f, &nobody, normals ? &nobody : nullptr};
  SmkVolGeom g;
  if (smk_volume_geometry(c, who, &b, 1, nelts, dtype, dmode, g)) return 1;
  free_volume(c);
  smk_set_geometry(c, g);
  c->ts.assign((size_t)c->ts_cap, TimeStep());
  TimeStep &T = c->ts[0];
  if (smk_alloc_step(c, g, T)) return 1;
  T.id = c->ts_cur_id;
  T.written = ++c->ts_written;
  const int none[3] = {0, 0, 0};
  HIPCHK(c, smk_pack_block(c, nullptr, nullptr, none, none, none, 0, 0, T, nullptr));
  HIPCHK(c, smk_bricks_minmax(T.vox, g.dtype, g.D, g.nbr, T.mm, nullptr));
  HIPCHK(c, hipDeviceSynchronize());
  T.vox_x_valid = false;
  T.valid_halo = c->halo;
  for (int a = 0; a < 3; ++a) {
    T.vlo[a] = g.O[a];
    T.vhi[a] = std::min(g.O[a] + g.D[a], g.N[a]);
  }
  smk_use_step(c, 0);
  c->tune_choice.clear();
  c->tune_sig = 0;
  return 0;
}

extern "C" int smk_set_clip(smk_ctx *c, int on, int oaxis, const float *vpos) {
  if (!c) return 1;
  if (!on) {
    c->clip_axis = 0;
    return 0;
  }
  if (oaxis < 1 || oaxis > 6 || !vpos) FAIL(c, "smk_set_clip: axis must be 1..6 (X+ X- Y+ Y- Z+ Z-) and vpos given");
  c->clip_axis = oaxis;
  for (int a = 0; a < 3; ++a) c->clip_vpos[a] = vpos[a];
  return 0;
}

extern "C" int smk_set_region(smk_ctx *c, int on, const float *lo, const float *hi) {
  if (!c) return 1;
  if (!on) {
    c->region_on = 0;
    return 0;
  }
  if (!lo || !hi) FAIL(c, "smk_set_region: null extents");
  for (int a = 0; a < 3; ++a) {
    c->region_lo[a] = lo[a] < hi[a] ? lo[a] : hi[a];
    c->region_hi[a] = lo[a] < hi[a] ? hi[a] : lo[a];
  }
  c->region_on = 1;
  return 0;
}

extern "C" int smk_set_clip_plane(smk_ctx *c, int on, const double *plane_eye) {
  if (!c) return 1;
  if (!on) {
    c->cplane_on = 0;
    return 0;
  }
  if (!plane_eye) FAIL(c, "smk_set_clip_plane: plane missing");
  c->cplane_on = 1;
  for (int k = 0; k < 4; ++k) c->cplane_eye[k] = plane_eye[k];
  return 0;
}

extern "C" int smk_set_shard(smk_ctx *c, int rank, int nranks) {
  if (!c) return 1;
  if (!(nranks == 1 || nranks == 2 || nranks == 4 || nranks == 8)) FAIL(c, "smk_set_shard: nranks must be 1,2,4 or 8");
  if (rank < 0 || rank >= nranks) FAIL(c, "smk_set_shard: rank out of range");
  if (c->have_volume) FAIL(c, "smk_set_shard: must be called before smk_upload_volume");
  c->rank = rank;
  c->nranks = nranks;
  return 0;
}

// ------------------------------------------------------------------------------- classification

template <class T>
static int dev_replace(smk_ctx *c, T **dptr, const void *host, size_t bytes) {
  if (*dptr) (void)hipFree(*dptr);
  *dptr = nullptr;
  HIPCHK(c, hipMalloc((void **)dptr, bytes));
  HIPCHK(c, hipMemcpy(*dptr, host, bytes, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int smk_set_tlut1d(smk_ctx *c, const float *rgba, int size) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!rgba || size < 2) FAIL(c, "smk_set_tlut1d: bad table");
  // TLUT::loadTransferTableRGBA (TLUT.cpp:65-71): theTable = (r*a, g*a, b*a, a)
  std::vector<float> t((size_t)size * 4);
  for (int n = 0; n < size; ++n) {
    float a = rgba[n * 4 + 3];
    t[n * 4 + 0] = rgba[n * 4 + 0] * a;
    t[n * 4 + 1] = rgba[n * 4 + 1] * a;
    t[n * 4 + 2] = rgba[n * 4 + 2] * a;
    t[n * 4 + 3] = a;
  }
  if (dev_replace(c, &c->d_tlut, t.data(), t.size() * 4)) return 1;
  c->tlut_size = size;
  c->tf_mode = 0;
  return 0;
}

extern "C" int smk_set_tf2d(smk_ctx *c, const unsigned char *deptex, const unsigned char *deptex2, int sv, int sg) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!deptex || sv < 2 || sg < 1) FAIL(c, "smk_set_tf2d: bad table");
  size_t bytes = (size_t)sv * sg * 4;
  c->h_tf_vg.assign(deptex, deptex + bytes);
  c->tf_raw_stale = true;
  if (deptex2) {
    c->h_tf_h.assign(deptex2, deptex2 + bytes);
    if (dev_replace(c, &c->d_tf_h, deptex2, bytes)) return 1;
  } else {
    c->h_tf_h.clear();
    if (c->d_tf_h) (void)hipFree(c->d_tf_h);
    c->d_tf_h = nullptr;
  }
  c->sv = sv;
  c->sg = sg;
  c->tf_mode = 1;
  c->tf_dirty = true;
  return 0;
}

extern "C" int smk_set_tf3d(smk_ctx *c, const unsigned char *ptex, int sv, int sg, int sh) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!ptex || sv < 1 || sg < 1 || sh < 1) FAIL(c, "smk_set_tf3d: bad table");
  if (dev_replace(c, &c->d_tf3d, ptex, (size_t)sv * sg * sh * 4)) return 1;
  // occupancy of the dense table, folded over its third axis: bit (t, s) is set when ANY sheet has a non-zero alpha in
  // the 2 x 2 texel quad based at (s, t).  A clear bit means the trilinear lookup of every sample whose (v, g) base texel
  // is (s, t) returns alpha == 0 exactly, whatever its third coordinate -- the kernels skip the eight-texel gather then
  // (the reference's widgets paint a few regions of a 256 x 256 x 4 table: most of it is transparent)
  {
    const int roww = (sv + 31) / 32;
    std::vector<uint32_t> occ((size_t)roww * sg, 0u);
    for (int t = 0; t < sg; ++t)
      for (int sx = 0; sx < sv; ++sx) {
        const int s1 = std::min(sx + 1, sv - 1), t1 = std::min(t + 1, sg - 1);
        unsigned any = 0;
        for (int h = 0; h < sh && !any; ++h) {
          const unsigned char *e = ptex + (size_t)h * sg * sv * 4;
          any = e[((size_t)t * sv + sx) * 4 + 3] | e[((size_t)t * sv + s1) * 4 + 3] | e[((size_t)t1 * sv + sx) * 4 + 3] | e[((size_t)t1 * sv + s1) * 4 + 3];
        }
        if (any) occ[(size_t)t * roww + (sx >> 5)] |= 1u << (sx & 31);
      }
    if (dev_replace(c, &c->d_tf3d_occ, occ.data(), occ.size() * 4)) return 1;
    c->tf3d_occ_roww = roww;
  }
  c->s3v = sv;
  c->s3g = sg;
  c->s3h = sh;
  c->tf_mode = 2;
  c->bricks3_dirty = true;
  return 0;
}

// ------------------------------------------------------------------------------- camera etc.

extern "C" int smk_set_camera(smk_ctx *c, const double mv[16], const float fr[4], const float clip[2], int w, int h) {
  if (!c) return 1;
  if (!mv || !fr || !clip) FAIL(c, "smk_set_camera: null argument");
  if (w <= 0 || h <= 0) FAIL(c, "smk_set_camera: bad window %dx%d", w, h);
  if (!(clip[0] > 0)) FAIL(c, "smk_set_camera: near plane must be > 0");
  if (!(fr[1] > fr[0]) || !(fr[3] > fr[2])) FAIL(c, "smk_set_camera: degenerate frustum");
  if ((w != c->W || h != c->H) && smk_present_outstanding(c))  // (a frame in flight owns buffers of the window it was begun with)
    FAIL(c, "smk_set_camera: the window cannot change from %dx%d to %dx%d while a frame of smk_render_present_begin is outstanding", c->W, c->H, w, h);
  memcpy(c->mv, mv, sizeof c->mv);
  memcpy(c->frustum, fr, sizeof c->frustum);
  memcpy(c->clip, clip, sizeof c->clip);
  c->W = w;
  c->H = h;
  c->have_camera = true;  // (steps-mode opacity correction follows the view-depth extent: refresh_tf2d compares the rate itself)
  return 0;
}

extern "C" int smk_set_shading(smk_ctx *c, smk_shade mode, const float lp[3], const float eye[3], const float at[3],
                               const float xf[16], float intens, float amb) {
  if (!c) return 1;
  if (mode < SMK_SHADE_NONE || mode > SMK_SHADE_NV20_DSPEC) FAIL(c, "smk_set_shading: bad mode");
  if (!lp || !eye || !at || !xf) FAIL(c, "smk_set_shading: null argument");
  c->shade = mode;
  memcpy(c->light_pos, lp, 12);
  memcpy(c->eye, eye, 12);
  memcpy(c->at, at, 12);
  memcpy(c->xform, xf, 64);
  c->intens = intens;
  c->amb = amb;
  return 0;
}

extern "C" int smk_set_sampling(smk_ctx *c, float rate, int steps, float gamma, int scale_alphas) {
  if (!c) return 1;
  if (steps <= 0 && !(rate > 0)) FAIL(c, "smk_set_sampling: need sample_rate > 0 or steps > 0");
  if (!(gamma > 0)) FAIL(c, "smk_set_sampling: gamma must be > 0");
  c->sample_rate = rate;
  c->steps = steps > 0 ? steps : 0;
  c->gamma = gamma;
  c->scale_alphas = scale_alphas;
  c->tf_dirty = true;
  return 0;
}

extern "C" int smk_set_blend(smk_ctx *c, smk_blend mode) {
  if (!c) return 1;
  if (mode < SMK_BLEND_FRONT_TO_BACK || mode > SMK_BLEND_MAX) FAIL(c, "smk_set_blend: bad mode");
  c->blend = mode;
  return 0;
}

extern "C" int smk_set_perturb(smk_ctx *c, const unsigned char *noise, int n, const float w[4], const float s[4]) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!noise || !w || !s || (w[0] == 0 && w[1] == 0)) {
    c->pw[0] = c->pw[1] = 0;
    return 0;
  }
  if (n < 1) FAIL(c, "smk_set_perturb: bad noise size");
  // a caller that sets the perturbation every frame (the adapter's draw()) hands over the same texture each time: the
  // device copy is replaced -- hipFree, hipMalloc and a synchronous copy, i.e. a device synchronisation -- only when the
  // bytes differ; weights and scales alone cost nothing
  const size_t nbytes = (size_t)n * n * n * 4;
  if (!(c->d_noise && c->nn == n && c->h_noise.size() == nbytes && !memcmp(c->h_noise.data(), noise, nbytes))) {
    if (dev_replace(c, &c->d_noise, noise, nbytes)) return 1;
    c->h_noise.assign(noise, noise + nbytes);
  }
  c->nn = n;
  memcpy(c->pw, w, 16);
  memcpy(c->ps, s, 16);
  return 0;
}

// ------------------------------------------------------------------------------- host setup

// VolumeRenderer::inverseMatrix (VolumeRenderer.cpp:1096-1131), affine, double
void smk_inverse_affine(double inv[16], const double m[16]) {
  double det = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[1] * m[4] * m[10] + m[1] * m[6] * m[8] +
               m[2] * m[4] * m[9] - m[2] * m[5] * m[8];
  inv[0] = (m[5] * m[10] - m[6] * m[9]) / det;
  inv[1] = (-m[1] * m[10] + m[2] * m[9]) / det;
  inv[2] = (m[1] * m[6] - m[2] * m[5]) / det;
  inv[3] = 0.0;
  inv[4] = (-m[4] * m[10] + m[6] * m[8]) / det;
  inv[5] = (m[0] * m[10] - m[2] * m[8]) / det;
  inv[6] = (-m[0] * m[6] + m[2] * m[4]) / det;
  inv[7] = 0.0;
  inv[8] = (m[4] * m[9] - m[5] * m[8]) / det;
  inv[9] = (-m[0] * m[9] + m[1] * m[8]) / det;
  inv[10] = (m[0] * m[5] - m[1] * m[4]) / det;
  inv[11] = 0.0;
  inv[12] = -(inv[0] * m[12] + inv[4] * m[13] + inv[8] * m[14]);
  inv[13] = -(inv[1] * m[12] + inv[5] * m[13] + inv[9] * m[14]);
  inv[14] = -(inv[2] * m[12] + inv[6] * m[13] + inv[10] * m[14]);
  inv[15] = 1.0;
}

// Sample placement of VolumeRenderer::render3DVA (VolumeRenderer.cpp:521-611) as ray
// coefficients: planes z_k = zmin + k*dis (k=1..S) perpendicular to view z, global for the whole
// volume (R8kVolRen3D.cpp:1331-1351); voxel coordinate of plane m (front to back) on the ray
// through pixel (i,j) is fma(m, B_a, A_a) with A,B affine in the pixel's frustum coordinates.
static int compute_raycoef(smk_ctx *c, smk_raycoef *o, double inv[16]) {
  smk_inverse_affine(inv, c->mv);
  const double *M = c->mv;
  double f[3] = {c->fsize[0], c->fsize[1], c->fsize[2]};
  double zmin = 1e300, zmax = -1e300;
  for (int i = 0; i < 8; ++i) {
    double x = (i & 1) ? f[0] : 0, y = (i & 2) ? f[1] : 0, z = (i & 4) ? f[2] : 0;
    double zz = M[2] * x + M[6] * y + M[10] * z + M[14];
    if (zz < zmin) zmin = zz;
    if (zz > zmax) zmax = zz;
  }
  double dist = zmax - zmin, dis;
  int S;
  if (c->steps > 0) {
    S = c->steps;
    dis = dist / S;
  } else {
    float disf = c->fsize[0] / ((float)c->N[0] * c->sample_rate);  // VolumeRenderer.cpp:595
    dis = disf;
    S = (int)(dist / dis);  // :598
  }
  if (S < 0) S = 0;
  double n = c->clip[0];
  double z0 = zmin + S * dis;
  double tau0 = -z0 / n, dtau = dis / n;
  double l = c->frustum[0], r = c->frustum[1], b = c->frustum[2], t = c->frustum[3];
  o->pxs = (float)((r - l) / c->W);
  o->pxl = (float)l;
  o->pys = (float)((t - b) / c->H);
  o->pyl = (float)b;
  double N[3] = {(double)c->N[0], (double)c->N[1], (double)c->N[2]};
  for (int a = 0; a < 3; ++a) {
    double s = N[a] / f[a];
    double R0 = inv[0 + a], R1 = inv[4 + a], R2 = inv[8 + a], e = inv[12 + a];
    o->Ac[a] = (float)((e - tau0 * n * R2) * s - 0.5);
    o->Ax[a] = (float)(tau0 * R0 * s);
    o->Ay[a] = (float)(tau0 * R1 * s);
    o->Bc[a] = (float)(-dtau * n * R2 * s);
    o->Bx[a] = (float)(dtau * R0 * s);
    o->By[a] = (float)(dtau * R1 * s);
  }
  o->nplanes = S;
  o->tau0 = (float)tau0;
  o->dtau = (float)dtau;
  o->zmin = (float)zmin;
  o->zmax = (float)zmax;
  o->dis = (float)dis;
  return 0;
}

extern "C" int smk_get_raycoef(smk_ctx *c, smk_raycoef *out) {
  if (!c || !out) return 1;
  if (!c->have_volume || !c->have_camera) FAIL(c, "smk_get_raycoef: volume and camera must be set");
  double inv[16];
  return compute_raycoef(c, out, inv);
}

static void normalize3(float v[3]) {
  float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (l > 0) {
    v[0] /= l;
    v[1] /= l;
    v[2] /= l;
  }
}

// light / half vectors: R8kVolRen3D::loadCubeTex (:2625-2640) or NV20VolRen3D::setupRegComb (:637-668)
static void shading_vectors(const smk_ctx *c, RenderParams &P) {
  const float *r = c->xform;
  // Nw = rows of xform . n (R8kVolRen3D.cpp:333-339)
  P.R[0] = r[0]; P.R[1] = r[4]; P.R[2] = r[8];
  P.R[3] = r[1]; P.R[4] = r[5]; P.R[5] = r[9];
  P.R[6] = r[2]; P.R[7] = r[6]; P.R[8] = r[10];
  P.intens = c->intens;
  P.use_spec = (c->shade == SMK_SHADE_R8K_DSPEC || c->shade == SMK_SHADE_NV20_DSPEC) ? 1 : 0;
  if (c->shade == SMK_SHADE_R8K_DIFF || c->shade == SMK_SHADE_R8K_DSPEC) {
    float l[3] = {-c->light_pos[0], -c->light_pos[1], -c->light_pos[2]};
    normalize3(l);
    float vd[3] = {-(c->eye[0] - c->at[0]), -(c->eye[1] - c->at[1]), -(c->eye[2] - c->at[2])};
    normalize3(vd);
    float h[3];
    for (int k = 0; k < 3; ++k) h[k] = l[k] + 0.5f * (vd[k] - l[k]);
    normalize3(h);
    memcpy(P.L, l, 12);
    memcpy(P.Hv, h, 12);
  } else {
    float vd[3] = {c->eye[0] - c->at[0], c->eye[1] - c->at[1], c->eye[2] - c->at[2]};
    normalize3(vd);
    float lt[3] = {c->light_pos[0] - c->at[0], c->light_pos[1] - c->at[1], c->light_pos[2] - c->at[2]};
    normalize3(lt);
    float h[3];
    for (int k = 0; k < 3; ++k) h[k] = lt[k] + 0.5f * (vd[k] - lt[k]);
    // through inverse(xform) (= transpose of the rotation), negated, normalised
    float hv[3] = {r[0] * h[0] + r[1] * h[1] + r[2] * h[2], r[4] * h[0] + r[5] * h[1] + r[6] * h[2],
                   r[8] * h[0] + r[9] * h[1] + r[10] * h[2]};
    float lv[3] = {r[0] * lt[0] + r[1] * lt[1] + r[2] * lt[2], r[4] * lt[0] + r[5] * lt[1] + r[6] * lt[2],
                   r[8] * lt[0] + r[9] * lt[1] + r[10] * lt[2]};
    for (int k = 0; k < 3; ++k) {
      hv[k] = -hv[k];
      lv[k] = -lv[k];
    }
    normalize3(hv);
    normalize3(lv);
    memcpy(P.L, lv, 12);
    memcpy(P.Hv, hv, 12);
  }
}

// brick flags of one table (smk_bricks.hip): buffers sized on demand, the two launches, the count copied back behind them
static int make_brick_set(smk_ctx *c, BrickSet &B, const uint32_t *occ, int roww, int sv, int sg, hipStream_t s) {
  const size_t nbricks = (size_t)c->nbr[0] * c->nbr[1] * c->nbr[2], sat_words = (size_t)(sv + 1) * (sg + 1);
  if (B.flags_cap < nbricks) {  // (a new volume size: rare; hipFree waits for the frames in flight)
    if (B.flags) (void)hipFree(B.flags);
    B.flags = nullptr;
    B.flags_cap = 0;
    HIPCHK(c, hipMalloc((void **)&B.flags, nbricks));
    B.flags_cap = nbricks;
  }
  if (B.sat_cap < sat_words) {
    if (B.sat) (void)hipFree(B.sat);
    B.sat = nullptr;
    B.sat_cap = 0;
    HIPCHK(c, hipMalloc((void **)&B.sat, sat_words * 4));
    B.sat_cap = sat_words;
  }
  if (!B.d_count) HIPCHK(c, hipMalloc((void **)&B.d_count, 4));
  if (!B.h_count) HIPCHK(c, hipHostMalloc((void **)&B.h_count, 4, hipHostMallocDefault));
  if (!B.counted) HIPCHK(c, hipEventCreateWithFlags(&B.counted, hipEventDisableTiming));
  else HIPCHK(c, hipEventSynchronize(B.counted));  // (the pinned word's previous copy: long done)
  if (smk_step_wait_ready(c, s)) return 1;  // (the summaries of a step uploaded asynchronously)
  HIPCHK(c, smk_bricks_flags(c->d_brick_mm, c->nbr, occ, roww, sv, sg, B.sat, B.flags, B.d_count, s));
  HIPCHK(c, hipMemcpyAsync(B.h_count, B.d_count, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipEventRecord(B.counted, s));
  B.valid = true;
  B.fill = -1.f;
  B.dil_r[0] = -1;  // (the dilated copy belongs to the old flags)
  return 0;
}

// the flags a frame should use, or null: none made, or (known by now) nearly every brick is flagged -- a table that
// leaves nothing to skip would only pay the flags' set-up in every workgroup
static const unsigned char *brick_flags_to_use(smk_ctx *c, BrickSet &B) {
  if (!B.valid) return nullptr;
  if (B.fill < 0.f && hipEventQuery(B.counted) == hipSuccess)
    B.fill = (float)((double)*B.h_count / ((double)c->nbr[0] * c->nbr[1] * c->nbr[2]));
  (void)hipGetLastError();
  return B.fill > 0.9f ? nullptr : B.flags;
}

// NV20VolRen3D::copyScale (:1645-1660) with the rate the renderer would pass (:94-98, :117)
// The effective (V,G) table of a frame: opacity correction as copyScale does it, plus the occupancy bitmap.  In steps
// mode the correction rate follows the view-depth extent, i.e. it changes with every camera move: the table is then
// rebuilt per frame, so the rebuild must neither stall the pipeline nor cost the host much.  The correction is a function
// of the alpha byte alone (a 256-entry map, same arithmetic as copyScale), so the host computes that map and a kernel
// applies it to the raw table kept on the device, writing the effective table and its bitmap into one of four versions
// (a version is rewritten only after the last frame that read it: an event wait ON THE STREAM, not on the host).
// Round 2 before: hipFree + hipMalloc + hipMemcpy per refresh = a device synchronisation and 1.6 ms of pow() per frame;
// then 65536 map look-ups + the bitmap on the host (0.4 ms per moving-camera frame, more than the launcher's planning).
__global__ __launch_bounds__(256) void smk_k_tf_effective(const uint32_t *raw, const unsigned char *map, int sv, int sg, int roww,
                                                           uint32_t *eff, uint32_t *occ) {
  // a wave = 64 consecutive texels of one row: its two bitmap words come from one ballot
  const int wave = (int)((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63;
  const int wpr = (sv + 63) / 64;  // waves per row
  const int t = wave / wpr, s = (wave - t * wpr) * 64 + lane;
  if (t >= sg) return;
  bool any = false;
  if (s < sv) {
    const int s1 = min(s + 1, sv - 1), t1 = min(t + 1, sg - 1);
    const uint32_t a = raw[(size_t)t * sv + s];
    const unsigned ma = map[a >> 24];
    eff[(size_t)t * sv + s] = (a & 0x00ffffffu) | (ma << 24);
    any = (ma | map[raw[(size_t)t * sv + s1] >> 24] | map[raw[(size_t)t1 * sv + s] >> 24] | map[raw[(size_t)t1 * sv + s1] >> 24]) != 0;
  }
  const unsigned long long m = __ballot(any);
  const int w0 = (s - lane) >> 5;
  if (lane == 0 && w0 < roww) occ[(size_t)t * roww + w0] = (uint32_t)m;
  if (lane == 32 && w0 + 1 < roww) occ[(size_t)t * roww + w0 + 1] = (uint32_t)(m >> 32);
}

static float tf2d_rate(const smk_ctx *c, const smk_raycoef &rc) {
  if (c->scale_alphas) {
    float rate = c->steps > 0 ? (float)(c->fsize[0] / ((double)c->N[0] * (double)rc.dis)) : c->sample_rate;
    return rate * 1 / c->gamma;
  }
  return 1 / c->gamma;
}

// NV20VolRen3D::copyScale (:1645-1660) per possible alpha byte
static void tf2d_alpha_map(const smk_ctx *c, float sr, unsigned char map[256]) {
  if (c->opt_tf_raw) {
    for (int a = 0; a < 256; ++a) map[a] = (unsigned char)a;
    return;
  }
  const float alphaScale = (float)(1.0 / sr);
  for (int a = 0; a < 256; ++a) map[a] = (unsigned char)(int)((1.0 - pow((1.0 - (a / 255.0)), alphaScale)) * 255);
}

static int refresh_tf2d(smk_ctx *c, const smk_raycoef &rc, hipStream_t frame_stream) {
  if (c->tf_mode != 1) return 0;
  const float sr = tf2d_rate(c, rc);
  if (!c->tf_dirty && sr == c->tf_rate_applied && c->d_tf_vg) {
    if (c->tf_ready_pending) HIPCHK(c, hipStreamWaitEvent(frame_stream, c->tf_ready, 0));  // (a no-op once the refresh has run)
    return 0;
  }
  // The correction is a function of the alpha BYTE: when the new rate maps every byte where the old one did -- a camera
  // that turns a little changes the view-depth extent in its fifth digit -- the effective table, its occupancy bitmap and
  // the brick flags would all come out byte for byte the same: nothing to refresh (a moving camera paid ~0.15 ms of
  // stream time per frame for these launches).
  unsigned char newmap[256];
  tf2d_alpha_map(c, sr, newmap);
  if (!c->tf_dirty && c->d_tf_vg && c->tf_map_valid && !memcmp(newmap, c->tf_map_applied, 256)) {
    c->tf_rate_applied = sr;
    if (c->tf_ready_pending) HIPCHK(c, hipStreamWaitEvent(frame_stream, c->tf_ready, 0));
    return 0;
  }
  // The refresh (alpha map copy, effective table + bitmap, summed-area table, brick flags: four small launches) runs on a
  // stream of its own and the frame's stream waits for its end: when the camera moves every frame the host enqueues frame
  // i + 1's refresh while frame i is still ray-marching, and the two overlap instead of queueing up behind one another.
  if (!c->tf_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->tf_stream, hipStreamNonBlocking));
  if (!c->tf_ready) HIPCHK(c, hipEventCreateWithFlags(&c->tf_ready, hipEventDisableTiming));
  const hipStream_t s = c->tf_stream;
  const size_t n = (size_t)c->sv * c->sg;
  const int sv = c->sv, sg = c->sg, roww = (sv + 31) / 32;
  const size_t occ_words = (size_t)roww * sg, bytes = n * 4 + occ_words * 4 + 256;  // table | bitmap | alpha map
  const int v = (c->tf_cur + 1) & 3;
  smk_ctx::TfVersion &T = c->tfv[v];
  if (T.cap < bytes) {  // (a new table size: rare)
    if (T.copied) (void)hipEventSynchronize(T.copied);
    if (T.used_valid) (void)hipEventSynchronize(T.used);
    if (T.d) (void)hipFree(T.d);
    if (T.h) (void)hipHostFree(T.h);
    T.d = nullptr;
    T.h = nullptr;
    T.cap = 0;
    HIPCHK(c, hipMalloc((void **)&T.d, bytes));
    HIPCHK(c, hipHostMalloc((void **)&T.h, bytes, hipHostMallocDefault));
    T.cap = bytes;
    if (!T.copied) HIPCHK(c, hipEventCreateWithFlags(&T.copied, hipEventDisableTiming));
    if (!T.used) HIPCHK(c, hipEventCreateWithFlags(&T.used, hipEventDisableTiming));
    T.used_valid = false;
  } else if (T.copied) {
    HIPCHK(c, hipEventSynchronize(T.copied));  // the staging buffer's previous copies (four refreshes ago) have run
  }
  // the raw table lives on the device; a new one travels through this version's staging buffer
  if (c->tf_raw_cap < n * 4) {
    HIPCHK(c, hipDeviceSynchronize());
    if (c->d_tf_raw) (void)hipFree(c->d_tf_raw);
    c->d_tf_raw = nullptr;
    c->tf_raw_cap = 0;
    HIPCHK(c, hipMalloc((void **)&c->d_tf_raw, n * 4));
    c->tf_raw_cap = n * 4;
    c->tf_raw_stale = true;
  }
  if (!c->tf_raw_ev) HIPCHK(c, hipEventCreateWithFlags(&c->tf_raw_ev, hipEventDisableTiming));
  if (c->tf_raw_stale) {
    memcpy(T.h, c->h_tf_vg.data(), n * 4);
    if (c->tf_raw_ev_valid) HIPCHK(c, hipStreamWaitEvent(s, c->tf_raw_ev, 0));  // the last kernel that read the old raw table is done
    HIPCHK(c, hipMemcpyAsync(c->d_tf_raw, T.h, n * 4, hipMemcpyHostToDevice, s));
    c->tf_raw_stale = false;
  }
  unsigned char *map = T.h + n * 4 + occ_words * 4;
  memcpy(map, newmap, 256);
  memcpy(c->tf_map_applied, newmap, 256);
  c->tf_map_valid = true;
  if (T.used_valid) HIPCHK(c, hipStreamWaitEvent(s, T.used, 0));  // the last frame that read this version is done
  HIPCHK(c, hipMemcpyAsync(T.d + n * 4 + occ_words * 4, map, 256, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipEventRecord(T.copied, s));
  // effective table + occupancy bitmap: bit (t, s) is set when any of the four texels a bilinear lookup with base texel
  // (s, t) touches has alpha != 0 after the correction.  A clear bit means the lookup returns alpha == 0 EXACTLY (lerps
  // of zeros), so a kernel may skip the fetch without changing a single bit of the frame.
  {
    const int wpr = (sv + 63) / 64;
    const unsigned blocks = (unsigned)(((size_t)wpr * sg + 3) / 4);
    hipLaunchKernelGGL(smk_k_tf_effective, dim3(blocks), dim3(256), 0, s, (const uint32_t *)c->d_tf_raw, T.d + n * 4 + occ_words * 4, sv,
                       sg, roww, (uint32_t *)T.d, (uint32_t *)(T.d + n * 4));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->tf_raw_ev, s));
    c->tf_raw_ev_valid = true;
  }
  c->tf_cur = v;
  c->d_tf_vg = reinterpret_cast<uint32_t *>(T.d);
  c->d_tf_occ = reinterpret_cast<uint32_t *>(T.d + n * 4);
  // this version's brick flags (smk_bricks.hip), behind the table on the same stream: two small launches per refresh
  T.br.valid = false;
  if (c->opt_bricks && c->d_brick_mm && make_brick_set(c, T.br, c->d_tf_occ, roww, sv, sg, s)) return 1;
  c->tf_occ_roww = roww;
  c->tf_rate_applied = sr;
  c->tf_dirty = false;
  HIPCHK(c, hipEventRecord(c->tf_ready, s));
  HIPCHK(c, hipStreamWaitEvent(frame_stream, c->tf_ready, 0));
  c->tf_ready_pending = true;
  return 0;
}

extern "C" int smk_get_tf2d_effective(smk_ctx *c, unsigned char *out, float *rate) {
  if (!c) return 1;
  if (c->tf_mode != 1 || !c->have_volume || !c->have_camera) FAIL(c, "smk_get_tf2d_effective: 2-D TF, volume and camera required");
  smk_raycoef rc;
  double inv[16];
  compute_raycoef(c, &rc, inv);
  if (refresh_tf2d(c, rc, c->stream)) return 1;
  if (out) {  // (the same map applied on the host: this call is for checkers, not for frames)
    unsigned char map[256];
    tf2d_alpha_map(c, c->tf_rate_applied, map);
    memcpy(out, c->h_tf_vg.data(), c->h_tf_vg.size());
    for (size_t i = 0; i < (size_t)c->sv * c->sg; ++i) out[i * 4 + 3] = map[c->h_tf_vg[i * 4 + 3]];
  }
  if (rate) *rate = c->tf_rate_applied;
  return 0;
}

// the shards in BSP order seen from a point (voxel index space): per split axis the half holding the point comes first
void smk_bsp_order(const smk_ctx *c, const double pos[3], int *order) {
  int nearbit[3];
  for (int a = 0; a < 3; ++a) nearbit[a] = pos[a] >= (double)(c->N[a] / 2) - 0.5 ? 1 : 0;
  int nbits = 0;
  for (int n = c->nranks; n > 1; n >>= 1) ++nbits;
  std::vector<std::pair<int, int>> keyed;
  for (int r = 0; r < c->nranks; ++r) {
    int key = 0;
    for (int bit = 0; bit < nbits; ++bit)
      if (((r >> bit) & 1) != nearbit[bit % 3]) key |= 1 << bit;
    keyed.push_back({key, r});
  }
  std::sort(keyed.begin(), keyed.end());
  for (int r = 0; r < c->nranks; ++r) order[r] = keyed[r].second;
}

extern "C" int smk_shard_order(smk_ctx *c, int *order) {
  if (!c || !order) return 1;
  if (!c->have_volume || !c->have_camera) FAIL(c, "smk_shard_order: volume and camera must be set");
  double inv[16];
  smk_inverse_affine(inv, c->mv);
  // eye in voxel index space
  double e[3];
  for (int a = 0; a < 3; ++a) e[a] = inv[12 + a] * c->N[a] / c->fsize[a] - 0.5;
  smk_bsp_order(c, e, order);
  return 0;
}

// ------------------------------------------------------------------------------- options and statistics

extern "C" int smk_set_option(smk_ctx *c, const char *key, int value) {
  if (!c || !key) return 1;
  if (!strcmp(key, "kernel")) c->opt_kernel = value;
  else if (!strcmp(key, "slab_T")) c->slab.opt_T = value & 0xff;
  else if (!strcmp(key, "inject_slab_status")) c->opt_inject_status = value;
  else if (!strcmp(key, "slab_fly")) c->slab.opt_fly = value < 0 ? 0 : (value > 63 ? 63 : value);
  else if (!strcmp(key, "slab_ns")) c->slab.opt_ns = value < 0 ? 0 : (value > 63 ? 63 : value);
  else if (!strcmp(key, "tile")) c->slab.opt_tile = value;
  else if (!strcmp(key, "shadow_march")) c->opt_shadow_march = value ? 1 : 0;  // (0: a launch per slice, the form of rounds 1-2)
  else if (!strcmp(key, "shadow_perturb")) c->opt_shadow_perturb = value ? 1 : 0;  // (opt-in: perturbed fetches under shadows, smk.h smk_set_shadow)
  else if (!strcmp(key, "shadow_look")) {  // 0: the R8k look; 1: the NV20 look of NV20VolRen3D2 (smk.h smk_set_shadow)
    if (value != 0 && value != 1) FAIL(c, "smk_set_option: shadow_look must be 0 (the R8k look) or 1 (the NV20 look)");
    c->opt_shadow_look = value;
  }
  else if (!strcmp(key, "shadow_fused")) c->opt_lockstep = value ? (c->opt_lockstep | 256) : (c->opt_lockstep & ~256);  // (developer: all slices in one cooperative launch)
  else if (!strcmp(key, "slab_split")) c->slab.opt_split = value < 0 ? 0 : (value > 8 ? 8 : value);
  else if (!strcmp(key, "cols_shape")) c->cols.opt_shape = value & 0xff;
  else if (!strcmp(key, "cols_ns")) c->cols.opt_ns = value & 0xff;
  else if (!strcmp(key, "cols_chunk")) c->cols.opt_chunk = value & 0xfff;
  else if (!strcmp(key, "cols_wstep")) c->cols.opt_wstep = value & 7;
  else if (!strcmp(key, "cols_counts")) c->cols.want_counts = value ? 1 : 0;
  else if (!strcmp(key, "cols_fill")) { c->cols.opt_fill = value; smk_cols_drop_layouts(&c->cols); }
  else if (!strcmp(key, "cols_take_min")) c->cols.opt_take_min = value;
  else if (!strcmp(key, "cols_take_wait")) c->cols.opt_take_wait = value;
  else if (!strcmp(key, "cols_fly")) c->cols.opt_fly = value;
  else if (!strcmp(key, "bricks")) {  // 0: the slice-ring kernel streams and samples every slice (smk_bricks.hip off)
    c->opt_bricks = value ? 1 : 0;
    c->tf_dirty = true;
    c->bricks3_dirty = true;
  }
  else if (!strcmp(key, "wave_w")) {
    if (!(value == 1 || value == 2 || value == 4 || value == 8 || value == 16 || value == 32 || value == 64)) FAIL(c, "smk_set_option: wave_w must be a power of two <= 64");
    c->opt_wave_w = value;
  } else if (!strcmp(key, "blk_w")) {
    if (!(value == 1 || value == 2 || value == 4)) FAIL(c, "smk_set_option: blk_w must be 1, 2 or 4");
    c->opt_blk_w = value;
  } else if (!strcmp(key, "lockstep")) c->opt_lockstep = value;
  else if (!strcmp(key, "tf_raw")) {  // the 2-D TF handed over is already opacity-corrected
    c->opt_tf_raw = value;
    c->tf_dirty = true;
  }
  else if (!strcmp(key, "halo")) {
    if (c->have_volume) FAIL(c, "smk_set_option: halo must be set before smk_upload_volume");
    if (value < 1) FAIL(c, "smk_set_option: halo must be >= 1");
    c->halo = value;
  } else
    FAIL(c, "smk_set_option: unknown key '%s'", key);
  return 0;
}

extern "C" int smk_get_brick_flags(smk_ctx *c, unsigned char *flags_out, int *nb_out, int *in_use_out) {
  if (!c || !nb_out) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  RenderParams P;
  if (smk_build_params(c, P, c->stream)) return 1;
  HIPCHK(c, hipDeviceSynchronize());
  for (int a = 0; a < 3; ++a) nb_out[a] = c->nbr[a];
  const BrickSet *B = c->tf_mode == 1 && c->tf_cur >= 0 ? &c->tfv[c->tf_cur].br : c->tf_mode == 2 ? &c->br3 : nullptr;
  if (in_use_out) *in_use_out = P.bricks != nullptr ? 1 : 0;
  if (flags_out) {
    if (!B || !B->valid || !B->flags) FAIL(c, "smk_get_brick_flags: no flags for this table (1-D colour table, or option 'bricks' 0)");
    HIPCHK(c, hipMemcpy(flags_out, B->flags, (size_t)c->nbr[0] * c->nbr[1] * c->nbr[2], hipMemcpyDeviceToHost));
  }
  return 0;
}

// a 64-bit device counter: zeroed, counted into by launch(d) on the context's stream, copied back; synchronises the stream
template <class Launch>
static int count_on_device(smk_ctx *c, Launch launch, double *out) {
  unsigned long long *d = nullptr, h = 0;
  HIPCHK(c, hipMalloc((void **)&d, 8));
  hipError_t e = hipMemsetAsync(d, 0, 8, c->stream);
  if (e == hipSuccess) e = launch(d);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  HIPCHK(c, e);
  *out = (double)h;
  return 0;
}

extern "C" int smk_get_stat(smk_ctx *c, const char *name, double *value) {
  if (!c || !name || !value) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  static const char *diag_names[SMK_SLAB_NDIAG] = {"slab_iters", "slab_active_lanes", "slab_inside_lanes", "slab_hit_lanes",
                                      "slab_loader_issue_kcyc", "slab_loader_wait_kcyc", "slab_loader_blocked_kcyc", "slab_loader_total_kcyc",
                                      "slab_iters_with_hit", "slab_lead_sum", "slab_waits", "slab_wstep_sum", "slab_dead_tail_sum", "slab_waves",
                                      "slab_iters_sampling", "slab_iters_own_brick",
                                      // turns with a lane on the visible path (occupancy bit set), that path's cycles, and those
                                      // of them spent waiting for the table texels (lockstep bit 512: waited for where issued)
                                      "slab_iters_with_maybe", "slab_visible_kcyc", "slab_texel_wait_kcyc"};
  for (int k = 0; k < SMK_SLAB_NDIAG; ++k)
    if (!strcmp(name, diag_names[k])) {
      float v = 0.f;
      if (c->slab.d_diag && read_back(c, &v, c->slab.d_diag + k, 1)) return 1;
      *value = v;
      return 0;
    }
  if (!strcmp(name, "light_samples")) {  // light-march samples of the current frame with shadows this context owns (all of them unsharded)
    RenderParams P;
    smk_shadowcoef sc;
    float olo[3], ohi[3];
    if (smk_shadow_light_owned(c, P, sc, olo, ohi)) return 1;
    return count_on_device(c, [&](unsigned long long *d) { return smk_launch_shadow_count_light(P, sc, olo, ohi, d, c->stream); }, value);
  }
  if (!strcmp(name, "slab_status")) {  // status word of the latest frame (0 = ok); synchronises
    HIPCHK(c, hipDeviceSynchronize());
    *value = c->slab.h_status ? (((volatile int *)c->slab.h_status)[c->slab.status_slot] & 0xff) : 0;
    return 0;
  }
  // frames the slice-ring kernel flagged invalid, as far as the host has looked (no synchronisation:
  // call after the frames of interest have completed); frames smk_render rendered a second time
  if (!strcmp(name, "slab_failures")) {
    long long n = c->slab_failures;
    if (c->slab.h_status)
      for (int k = 0; k < SMK_STATUS_RING; ++k) n += ((volatile int *)c->slab.h_status)[k] != 0;
    *value = (double)n;
    return 0;
  }
  // share of the slices in the tiles' ranges that the loaders of the latest slice-ring frame really
  // streamed (they stop when every ray of a tile is saturated); synchronises
  if (!strcmp(name, "slab_streamed_fraction")) {
    *value = 1.0;
    const int nt = c->slab.ticks_n_last;
    if (c->last_kernel == 2 && c->slab.d_ticks && nt > 0) {
      std::vector<unsigned> h((size_t)2 * nt);
      if (read_back(c, h.data(), c->slab.d_ticks + nt, h.size())) return 1;
      double st = 0, pl = 0;
      for (int t = 0; t < nt; ++t) {
        st += h[t];
        pl += h[(size_t)nt + t];
      }
      if (pl > 0) *value = st / pl;
    }
    return 0;
  }
  // longest and summed workgroup durations of the latest slice-ring frame, in ms (the kernel's per-tile ticks); synchronises
  if (!strcmp(name, "slab_tile_ms_max") || !strcmp(name, "slab_tile_ms_sum")) {
    *value = 0.0;
    const int nt = c->slab.ticks_n_last;
    if (c->last_kernel == 2 && c->slab.d_ticks && nt > 0) {
      std::vector<unsigned> h((size_t)nt);
      if (read_back(c, h.data(), c->slab.d_ticks, h.size())) return 1;
      double mx = 0, sum = 0;
      for (int t = 0; t < nt; ++t) {
        // (a split tile's word is the sum over its pieces: the longest workgroup is taken as an equal share)
        const double k = t < (int)c->slab.ksplit_last.size() ? std::max<int>(c->slab.ksplit_last[t], 1) : 1;
        mx = std::max(mx, (double)h[t] / k);
        sum += h[t];
      }
      *value = (name[13] == 'm' ? mx : sum) * 1e-5;  // 100 MHz ticks
    }
    return 0;
  }
  if (!strncmp(name, "cols_", 5)) return smk_cols_stat(c, name, value);  // column-stream kernel (smk_cols_plan.hip)
  if (!strncmp(name, "slab_plan_", 10)) return smk_slab_plan_stat(c, name, value);  // the latest slice-ring launch's plan (smk_slab_plan.hip)
  if (!strcmp(name, "slab_split_tiles")) { *value = c->slab.nsplit_last; return 0; }
  if (!strcmp(name, "slab_workgroups")) { *value = c->slab.nblocks_last; return 0; }
  if (!strcmp(name, "slab_retries")) { *value = (double)c->slab_retries; return 0; }
  if (!strcmp(name, "clip_slice_pass")) { *value = c->clip_slice_pass; return 0; }  // (smk_clip_slice.hip)
  // the hand-over to the host (smk_present.hip): the present kernel's HIP-event time of the last frame handed over (after
  // smk_present_device: waits for it), and the bytes that frame's copy to the host moved
  if (!strcmp(name, "present_ms")) return smk_present_ms(c, value);
  if (!strcmp(name, "present_bytes")) { *value = c->present_bytes; return 0; }
  if (!strcmp(name, "tblend_count")) { *value = (double)c->tblend_count; return 0; }
  FAIL(c, "smk_get_stat: unknown name '%s'", name);
}

extern "C" int smk_get_trace(smk_ctx *c, unsigned *out, int cap_records, int *nrecords) {
  if (!c || !nrecords) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!(c->opt_lockstep & 32)) {
    // no diagnostic instance ran: the product kernel's own words per tile (start, duration, where) in the same record shape
    const int nt = c->last_kernel == 2 && c->slab.d_ticks ? c->slab.ticks_n_last : 0;
    *nrecords = nt;
    if (out && nt > 0) {
      std::vector<unsigned> h((size_t)nt * 5);
      if (read_back(c, h.data(), c->slab.d_ticks, h.size())) return 1;
      for (int t = 0; t < std::min(cap_records, nt); ++t) {
        unsigned *r = out + (size_t)t * 8;
        r[0] = h[(size_t)3 * nt + t];
        r[1] = h[(size_t)3 * nt + t] ? r[0] + h[t] : 0u;   // (a tile cut in depth segments has no start word: record left empty)
        r[2] = h[(size_t)4 * nt + t] & 0xff00u;
        r[3] = (h[(size_t)4 * nt + t] & 0xfu) | ((unsigned)t << 8) | (h[(size_t)2 * nt + t] << 20);
        r[4] = r[5] = r[6] = r[7] = 0;
      }
    }
    return 0;
  }
  *nrecords = c->slab.d_trace ? c->slab.trace_n : 0;
  if (out && *nrecords > 0 && read_back(c, out, c->slab.d_trace, (size_t)std::min(cap_records, *nrecords) * 8)) return 1;
  return 0;
}

extern "C" int smk_count_samples(smk_ctx *c, double *in_volume) {
  if (!c || !in_volume) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  RenderParams P;
  if (smk_build_params(c, P, c->stream)) return 1;
  // a frame with shadows samples the half-angle slices in its eye box (smk_shadow_setup)
  smk_shadowcoef sc;
  // (perturbation displaces the fetch, not the sample: it changes no count; a sub-box is in the boxes)
  if (c->shadow_on && c->tf_mode != 0 && smk_shadow_setup(c, P, sc, nullptr, nullptr)) return 1;
  return count_on_device(c, [&](unsigned long long *d) { return smk_launch_count_inside(P, d, c->stream); }, in_volume);
}

// The box of voxels g0..g1 in voxel coordinates, [g0 - .5, g1 - .5) per axis (closed where top[a]: the volume's upper face),
// cut by an orthogonal clip plane and the sub-box.  A shard's region; with 0..N the whole volume's box.
void smk_region_box(const smk_ctx *c, const int g0[3], const int g1[3], float lo[3], float hi[3], int top[3]) {
  for (int a = 0; a < 3; ++a) {
    lo[a] = (float)g0[a] - 0.5f;
    hi[a] = (float)g1[a] - 0.5f;
    top[a] = g1[a] == c->N[a];
  }
  // orthogonal clip plane (NV20VolRen3D::setupClips, NV20VolRen3D.cpp:251-327): the sliced box ends
  // at the plane, i.e. the region shrinks along one axis; the new face is an outer (inclusive) one
  if (c->clip_axis >= 1 && c->clip_axis <= 6) {
    const int a = (c->clip_axis - 1) / 2;
    const float fs = c->fsize[a];
    const float cp = c->clip_vpos[a] > 0.0f ? (c->clip_vpos[a] < fs ? c->clip_vpos[a] : fs) : 0.0f;
    const float face = (float)((double)cp / (double)fs * (double)c->N[a] - 0.5);
    if ((c->clip_axis - 1) % 2 == 0) {
      if (face < hi[a] || (face == hi[a] && !top[a])) { hi[a] = face; top[a] = 1; }
    } else if (face > lo[a]) {
      lo[a] = face;
    }
  }
  // sub-box of renderVolume(.., xext, yext, zext) (VolumeRenderer.cpp:428-505): the region shrinks on every axis; the new
  // upper faces are half-open like a shard's inner ones (a face that coincides with a voxel plane belongs to one side)
  if (c->region_on)
    for (int a = 0; a < 3; ++a) {
      const double fs = c->fsize[a];
      const double l = c->region_lo[a] > 0 ? (c->region_lo[a] < fs ? c->region_lo[a] : fs) : 0.0;
      const double h = c->region_hi[a] > 0 ? (c->region_hi[a] < fs ? c->region_hi[a] : fs) : 0.0;
      const float flo = (float)(l / fs * (double)c->N[a] - 0.5), fhi = (float)(h / fs * (double)c->N[a] - 0.5);
      if (flo > lo[a]) lo[a] = flo;
      if (fhi < hi[a]) { hi[a] = fhi; top[a] = 0; }
    }
}

int smk_build_params(smk_ctx *c, RenderParams &P, hipStream_t s) {
  if (!c->have_volume) FAIL(c, "smk_render: no volume uploaded");
  if (!c->have_camera) FAIL(c, "smk_render: no camera set");
  if (c->tf_mode < 0) FAIL(c, "smk_render: no transfer function set");
  memset(&P, 0, sizeof P);
  double inv[16];
  compute_raycoef(c, &P.rc, inv);
  if (refresh_tf2d(c, P.rc, s)) return 1;
  if (smk_step_wait_ready(c, s)) return 1;  // a time step uploaded on another stream: the frame waits for it there
  P.vox = c->d_vox;
  P.nrm = c->d_nrm;
  for (int a = 0; a < 3; ++a) {
    P.N[a] = c->N[a];
    P.O[a] = c->O[a];
    P.D[a] = c->D[a];
    P.invN[a] = 1.0f / (float)c->N[a];
  }
  smk_region_box(c, c->g0, c->g1, P.lo, P.hi, P.top);
  for (int a = 0; a < 3; ++a) P.hin[a] = P.top[a] ? P.hi[a] : nextafterf(P.hi[a], -INFINITY);
  // free clip plane: eye-space plane -> voxel coordinates.  eye = MV * model, model = (p + 1/2)/N * fSize
  // (same operations in the same order as the CPU checker's orc_clip_plane_voxel)
  P.cplane_on = c->cplane_on;
  for (int k = 0; k < 4; ++k) P.cplane[k] = 0.0f;
  if (c->cplane_on) {
    double pm[4];  // plane in model space: row vector times MV (column-major)
    for (int k = 0; k < 4; ++k)
      pm[k] = c->cplane_eye[0] * c->mv[4 * k + 0] + c->cplane_eye[1] * c->mv[4 * k + 1] + c->cplane_eye[2] * c->mv[4 * k + 2] +
              c->cplane_eye[3] * c->mv[4 * k + 3];
    double w = pm[3];
    for (int a = 0; a < 3; ++a) {
      const double sc = (double)c->fsize[a] / (double)c->N[a];
      P.cplane[a] = (float)(pm[a] * sc);
      w += pm[a] * sc * 0.5;
    }
    P.cplane[3] = (float)w;
  }
  P.nelts = c->nelts;
  P.n_in_w = (c->dtype == SMK_F32 && c->nelts <= 3) ? 1 : 0;
  P.tlut = c->d_tlut;
  P.tlut_size = c->tlut_size;
  P.tf_vg = c->d_tf_vg;
  P.tf_h = c->d_tf_h;
  P.tf_occ = c->tf_mode == 1 ? c->d_tf_occ : c->tf_mode == 2 ? c->d_tf3d_occ : nullptr;
  P.occ_roww = c->tf_mode == 2 ? c->tf3d_occ_roww : c->tf_occ_roww;
  P.sv = c->sv;
  P.sg = c->sg;
  // third-axis data modes (NV20VolRen3D.cpp:686-693, 813-819)
  bool third = c->dmode == SMK_GDM_VGH || c->dmode == SMK_GDM_V1GH || c->dmode == SMK_GDM_V2G ||
               c->dmode == SMK_GDM_V2GH || c->dmode == SMK_GDM_V3 || c->dmode == SMK_GDM_V3G || c->dmode == SMK_GDM_V4;
  P.third_axis = (third && c->d_tf_h && c->nelts >= 3) ? 1 : 0;
  P.tf3d = c->d_tf3d;
  P.s3v = c->s3v;
  P.s3g = c->s3g;
  P.s3h = c->s3h;
  // brick flags (smk_bricks.hip): the 2-D table's come with its version; the dense 3-D table's are made here when stale
  P.bricks = nullptr;
  for (int a = 0; a < 3; ++a) P.nbr[a] = c->nbr[a];
  BrickSet *bset = nullptr;
  P.bricks_dil = nullptr;
  if (c->opt_bricks && c->d_brick_mm) {
    if (c->tf_mode == 1 && c->tf_cur >= 0) {
      P.bricks = brick_flags_to_use(c, c->tfv[c->tf_cur].br);
      bset = &c->tfv[c->tf_cur].br;
    }
    if (c->tf_mode == 2 && c->d_tf3d_occ) {
      if (c->bricks3_dirty || !c->br3.valid) {
        HIPCHK(c, hipDeviceSynchronize());  // (a new table or volume: rare; frames in flight may still read the old flags)
        if (make_brick_set(c, c->br3, c->d_tf3d_occ, c->tf3d_occ_roww, c->s3v, c->s3g, s)) return 1;
        c->bricks3_dirty = false;
      }
      P.bricks = brick_flags_to_use(c, c->br3);
      bset = &c->br3;
    }
  }
  P.W = c->W;
  P.H = c->H;
  P.znear = c->clip[0];
  shading_vectors(c, P);
  P.blend = c->blend;
  P.noise = c->d_noise;
  P.nn = c->nn;
  P.nn_log2 = -1;
  for (int l = 0; l < 12; ++l)
    if (c->nn == (1 << l)) P.nn_log2 = l;
  P.pw[0] = c->pw[0];
  P.pw[1] = c->pw[1];
  P.ps[0] = c->ps[0];
  P.ps[1] = c->ps[1];
  P.pert_on = (c->d_noise && (c->pw[0] != 0 || c->pw[1] != 0)) ? 1 : 0;
  if (P.pert_on && c->nranks > 1) {
    // a displaced fetch must stay inside region + halo: the halo voxels of the SHOWN step that are exact (a sharded stencil
    // producer leaves fewer than it found)
    const int have = smk_step_shown_halo(c);
    for (int a = 0; a < 3; ++a) {
      int need = 1 + (int)ceil(0.5 * (fabs(c->pw[0]) + fabs(c->pw[1])) * c->N[a]);
      if (have < need && c->D[a] < c->N[a]) {
        if (have != c->halo)
          FAIL(c, "smk_render: perturbation needs halo >= %d voxels on a sharded volume (time step %d has a valid halo of %d, of option halo %d: "
                  "smk_get_timestep_halo); set option 'halo' before upload", need, c->ts_cur_id, have, c->halo);
        FAIL(c, "smk_render: perturbation needs halo >= %d voxels on a sharded volume (have %d); set option 'halo' before upload", need, c->halo);
      }
    }
  }
  // a perturbed fetch lands within 0.5 (|w0| + |w1|) N voxels of the undisplaced position on every axis: when that is a
  // brick or two, flags spread that far tell BEFORE the noise lookups that nothing visible can be reached
  if (P.pert_on && P.bricks && bset) {
    int r[3];
    bool near = true;
    for (int a = 0; a < 3; ++a) {
      const int dv = (int)ceil(0.5 * (fabs(c->pw[0]) + fabs(c->pw[1])) * c->N[a] + 1e-3);
      r[a] = (dv + (1 << SMK_BRICK_LOG2) - 1) >> SMK_BRICK_LOG2;
      near = near && r[a] <= 2;
    }
    if (near) {
      const size_t nbricks = (size_t)c->nbr[0] * c->nbr[1] * c->nbr[2];
      if (bset->dil_cap < nbricks) {
        if (bset->dil) (void)hipFree(bset->dil);
        bset->dil = nullptr;
        bset->dil_cap = 0;
        HIPCHK(c, hipMalloc((void **)&bset->dil, nbricks));
        bset->dil_cap = nbricks;
        bset->dil_r[0] = -1;
      }
      if (bset->dil_r[0] != r[0] || bset->dil_r[1] != r[1] || bset->dil_r[2] != r[2]) {
        HIPCHK(c, smk_bricks_dilate(bset->flags, c->nbr, r, bset->dil, s));
        for (int a = 0; a < 3; ++a) bset->dil_r[a] = r[a];
      }
      P.bricks_dil = bset->dil;
    }
  }
  P.wave_w = c->opt_wave_w;
  P.blk_w = c->opt_blk_w;
  P.lockstep = c->opt_lockstep;
  int tw = P.wave_w * P.blk_w, th = (64 / P.wave_w) * (4 / P.blk_w);
  P.ntx = (c->W + tw - 1) / tw;
  P.nty = (c->H + th - 1) / th;
  P.tiles_per_xcd = (P.ntx * P.nty + 7) / 8;
  return 0;
}

// [z][y][x] -> [x][z][y] so that views along x also read contiguous rows (288 GB of HBM buys a
// second layout; only one copy is read per frame).  32x32 tiles through LDS keep both sides
// coalesced in 16-byte (f32: 2 x 8-byte) units.
template <class V>
__global__ __launch_bounds__(256) void smk_k_xmajor(const V *src, V *dst, int Dx, int Dy, int Dz) {
  __shared__ V tile[32][33];
  int z = blockIdx.z, x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
  int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) {
    int x = x0 + tx, y = y0 + r;
    if (x < Dx && y < Dy) tile[r][tx] = src[((size_t)z * Dy + y) * Dx + x];
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    int x = x0 + r, y = y0 + tx;
    if (x < Dx && y < Dy) dst[((size_t)x * Dz + z) * Dy + y] = tile[tx][r];
  }
}

int smk_make_xmajor_copy(smk_ctx *c) {
  if (c->d_vox_x) return 0;
  TimeStep &T = c->ts[c->ts_cur];  // (the current step's copy: made once per upload of the step)
  if (!T.vox_x) HIPCHK(c, hipMalloc(&T.vox_x, c->vox_bytes));
  c->d_vox_x = T.vox_x;
  if (smk_step_wait_ready(c, c->stream)) return 1;
  dim3 grid((c->D[0] + 31) / 32, (c->D[1] + 31) / 32, c->D[2]);
  if (c->dtype != SMK_F32)  // (by voxel size: u8 and u16 voxels are 8 bytes)
    hipLaunchKernelGGL(smk_k_xmajor<uint2>, grid, dim3(256), 0, c->stream, (const uint2 *)c->d_vox, (uint2 *)c->d_vox_x,
                       c->D[0], c->D[1], c->D[2]);
  else
    hipLaunchKernelGGL(smk_k_xmajor<float4>, grid, dim3(256), 0, c->stream, (const float4 *)c->d_vox,
                       (float4 *)c->d_vox_x, c->D[0], c->D[1], c->D[2]);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.vox_x_valid = true;
  return 0;
}

int smk_shade_kind(const smk_ctx *c) {
  if (c->tf_mode == 0 || !c->have_normals) return 0;
  if (c->shade == SMK_SHADE_R8K_DIFF || c->shade == SMK_SHADE_R8K_DSPEC) return 1;
  if (c->shade == SMK_SHADE_NV20_DIFF || c->shade == SMK_SHADE_NV20_DSPEC) return 2;
  return 0;
}

// ------------------------------------------------------------------------------- renderSlice

// VolumeRenderer::render3dSliceEXT (VolumeRenderer.cpp:762-807): one textured quad blended into the frame.  A thread per
// pixel: the ray through the pixel centre against the quad's two triangles (vertices in GL's order 1, 0, 2, 3 -> (a, b, c),
// (a, c, d)); texture coordinates are vertex / fSize, i.e. linear in the model-space position, so the perspective-correct
// interpolation GL does IS the hit point.  Sampling as the ray-marchers do: GL_LINEAR, clamp to edge, channel 0.
struct SliceArg {
  float v[4][3];   // quad vertices in voxel coordinates (x / fSize * N - 0.5), order a, b, c, d
  float alpha;
};

template <int DT>
__global__ __launch_bounds__(256) void smk_k_render_slice(const RenderParams P, const SliceArg Q, float4 *fb) {
  const int i = blockIdx.x * 16 + (threadIdx.x & 15), j = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i >= P.W || j >= P.H) return;
  const smk_raycoef &rc = P.rc;
  const float px = __fmaf_rn((float)i + 0.5f, rc.pxs, rc.pxl), py = __fmaf_rn((float)j + 0.5f, rc.pys, rc.pyl);
  float A[3], B[3];
  for (int a = 0; a < 3; ++a) {
    A[a] = __fmaf_rn(px, rc.Ax[a], __fmaf_rn(py, rc.Ay[a], rc.Ac[a]));
    B[a] = __fmaf_rn(px, rc.Bx[a], __fmaf_rn(py, rc.By[a], rc.Bc[a]));
  }
  // eye = A - (tau0 / dtau) B (every ray starts there); direction B
  const float k = rc.tau0 / rc.dtau;
  const float O[3] = {A[0] - k * B[0], A[1] - k * B[1], A[2] - k * B[2]};
  bool hit = false;
  float X[3] = {0, 0, 0};
  for (int t = 0; t < 2 && !hit; ++t) {
    const float *v0 = Q.v[0], *v1 = Q.v[t == 0 ? 1 : 2], *v2 = Q.v[t == 0 ? 2 : 3];
    const float e1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]}, e2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    const float pv[3] = {B[1] * e2[2] - B[2] * e2[1], B[2] * e2[0] - B[0] * e2[2], B[0] * e2[1] - B[1] * e2[0]};
    const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
    if (fabsf(det) < 1e-20f) continue;
    const float inv = 1.0f / det;
    const float tv[3] = {O[0] - v0[0], O[1] - v0[1], O[2] - v0[2]};
    const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * inv;
    const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
    const float w = (B[0] * qv[0] + B[1] * qv[1] + B[2] * qv[2]) * inv;
    const float tt = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * inv;
    if (u < 0.0f || w < 0.0f || u + w > 1.0f || !(tt * rc.dtau > 0.0f)) continue;  // (in front of the eye)
    hit = true;
    for (int a = 0; a < 3; ++a) X[a] = v0[a] + u * e1[a] + w * e2[a];
  }
  if (!hit) return;
  int x0, x1, y0, y1, z0, z1;
  float fx, fy, fz;
  smk_lin_clamp(X[0], P.N[0], x0, x1, fx);
  smk_lin_clamp(X[1], P.N[1], y0, y1, fy);
  smk_lin_clamp(X[2], P.N[2], z0, z1, fz);
  x0 = min(max(x0 - P.O[0], 0), P.D[0] - 1); x1 = min(max(x1 - P.O[0], 0), P.D[0] - 1);
  y0 = min(max(y0 - P.O[1], 0), P.D[1] - 1); y1 = min(max(y1 - P.O[1], 0), P.D[1] - 1);
  z0 = min(max(z0 - P.O[2], 0), P.D[2] - 1); z1 = min(max(z1 - P.O[2], 0), P.D[2] - 1);
  const size_t Dx = P.D[0], Dy = P.D[1];
  auto at = [&](int x, int y, int z) -> float { return smk_load_corner<DT>(P, ((size_t)z * Dy + y) * Dx + x).c0; };
  float I = smk_lerp(smk_lerp(smk_lerp(at(x0, y0, z0), at(x1, y0, z0), fx), smk_lerp(at(x0, y1, z0), at(x1, y1, z0), fx), fy),
                     smk_lerp(smk_lerp(at(x0, y0, z1), at(x1, y0, z1), fx), smk_lerp(at(x0, y1, z1), at(x1, y1, z1), fx), fy), fz);
  if (DT != 1) I *= SmkScale<DT>::s01;
  I = smk_sat(I);
  const float sa = smk_sat(I * Q.alpha);
  float4 D = fb[(size_t)j * P.W + i];
  const float w1 = 1.0f - sa;
  D.x = __fmaf_rn(w1, D.x, I);
  D.y = __fmaf_rn(w1, D.y, I);
  D.z = __fmaf_rn(w1, D.z, I);
  D.w = __fmaf_rn(w1, D.w, sa);
  fb[(size_t)j * P.W + i] = D;
}

extern "C" int smk_render_slice_device(smk_ctx *c, const float quad[4][3], float alpha, void *d_rgba, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!quad || !d_rgba) FAIL(c, "smk_render_slice: null argument");
  if (!c->have_volume) FAIL(c, "smk_render_slice: no volume uploaded");
  if (!c->have_camera) FAIL(c, "smk_render_slice: no camera set");
  if (c->nranks > 1) FAIL(c, "smk_render_slice: the slice quad is drawn from the whole volume (unsharded context)");
  RenderParams P;
  memset(&P, 0, sizeof P);
  double inv[16];
  compute_raycoef(c, &P.rc, inv);
  P.vox = c->d_vox;
  P.nrm = c->d_nrm;
  for (int a = 0; a < 3; ++a) { P.N[a] = c->N[a]; P.O[a] = c->O[a]; P.D[a] = c->D[a]; }
  P.nelts = c->nelts;
  P.n_in_w = (c->dtype == SMK_F32 && c->nelts <= 3) ? 1 : 0;
  P.W = c->W;
  P.H = c->H;
  SliceArg Q;
  const int ord[4] = {1, 0, 2, 3};  // glVertex order of render3dSliceEXT (:776-792)
  for (int k = 0; k < 4; ++k)
    for (int a = 0; a < 3; ++a) Q.v[k][a] = (float)((double)quad[ord[k]][a] / (double)c->fsize[a] * (double)c->N[a] - 0.5);
  Q.alpha = alpha;
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  dim3 grid((c->W + 15) / 16, (c->H + 15) / 16);
  if (smk_step_wait_ready(c, s)) return 1;
  if (c->dtype == SMK_U8) hipLaunchKernelGGL(smk_k_render_slice<0>, grid, dim3(256), 0, s, P, Q, (float4 *)d_rgba);
  else if (c->dtype == SMK_U16) hipLaunchKernelGGL(smk_k_render_slice<2>, grid, dim3(256), 0, s, P, Q, (float4 *)d_rgba);
  else hipLaunchKernelGGL(smk_k_render_slice<1>, grid, dim3(256), 0, s, P, Q, (float4 *)d_rgba);
  HIPCHK(c, hipGetLastError());
  return smk_step_mark_used(c, s);
}

extern "C" int smk_render_slice(smk_ctx *c, const float quad[4][3], float alpha, float *rgba) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!rgba) FAIL(c, "smk_render_slice: null frame");
  if (!c->have_camera) FAIL(c, "smk_render_slice: no camera set");
  const size_t npix = (size_t)c->W * c->H;
  if (smk_frame_buffers(c)) return 1;
  HIPCHK(c, hipMemcpy(c->d_out, rgba, npix * 16, hipMemcpyHostToDevice));
  if (smk_render_slice_device(c, quad, alpha, c->d_out, c->stream)) return 1;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(rgba, c->d_out, npix * 16, hipMemcpyDeviceToHost));
  return 0;
}

// ------------------------------------------------------------------------------- sort-last merge

struct OrderArg {
  int o[SMK_MAX_RANKS];
};

// DEPTH: the depth layers merge in the same pass, by minimum (a template flag: the RGBA loop is the same code either way)
template <bool DEPTH>
__global__ void smk_k_over(const float4 *layers, const float *depths, int nlayers, OrderArg ord, int npix, float4 *out,
                           float *depth_out, int use_max) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npix) return;
  float4 C = make_float4(0.f, 0.f, 0.f, 0.f);
  float Z = __int_as_float(0x7f800000);
  for (int l = 0; l < nlayers; ++l) {
    float4 s = layers[(size_t)ord.o[l] * npix + p];
    if (DEPTH) Z = fminf(Z, depths[(size_t)ord.o[l] * npix + p]);
    if (use_max) {  // GL_MAX layers merge by maximum, in any order
      C = make_float4(fmaxf(C.x, s.x), fmaxf(C.y, s.y), fmaxf(C.z, s.z), fmaxf(C.w, s.w));
      continue;
    }
    float w = 1.0f - C.w;
    C.x = __fmaf_rn(w, s.x, C.x);
    C.y = __fmaf_rn(w, s.y, C.y);
    C.z = __fmaf_rn(w, s.z, C.z);
    C.w = __fmaf_rn(w, s.w, C.w);
  }
  out[p] = C;
  if (DEPTH) depth_out[p] = Z;
}

static int composite_over(smk_ctx *c, const char *fn, const void *d_layers, const void *d_depths, int nlayers, const int *order,
                          int npix, void *d_out, void *d_depth_out, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!d_layers || !d_out || !order) FAIL(c, "%s: null argument", fn);
  if (nlayers < 1 || nlayers > SMK_MAX_RANKS) FAIL(c, "%s: 1..%d layers", fn, SMK_MAX_RANKS);
  OrderArg oa;
  for (int l = 0; l < nlayers; ++l) {
    if (order[l] < 0 || order[l] >= nlayers) FAIL(c, "%s: order[%d]=%d out of range", fn, l, order[l]);
    oa.o[l] = order[l];
  }
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const int use_max = c->blend == SMK_BLEND_MAX ? 1 : 0;
  if (d_depths)
    hipLaunchKernelGGL(smk_k_over<true>, dim3((npix + 255) / 256), dim3(256), 0, s, (const float4 *)d_layers, (const float *)d_depths,
                       nlayers, oa, npix, (float4 *)d_out, (float *)d_depth_out, use_max);
  else
    hipLaunchKernelGGL(smk_k_over<false>, dim3((npix + 255) / 256), dim3(256), 0, s, (const float4 *)d_layers, (const float *)nullptr,
                       nlayers, oa, npix, (float4 *)d_out, (float *)nullptr, use_max);
  HIPCHK(c, hipGetLastError());
  return 0;
}

extern "C" int smk_composite_over_device(smk_ctx *c, const void *d_layers, int nlayers, const int *order, int npix,
                                         void *d_out, void *stream) {
  return composite_over(c, "smk_composite_over_device", d_layers, nullptr, nlayers, order, npix, d_out, nullptr, stream);
}

extern "C" int smk_composite_over_depth_device(smk_ctx *c, const void *d_layers, const void *d_depths, int nlayers, const int *order,
                                               int npix, void *d_out, void *d_depth_out, void *stream) {
  if (c && (!d_depths || !d_depth_out)) FAIL(c, "smk_composite_over_depth_device: null depth argument");
  return composite_over(c, "smk_composite_over_depth_device", d_layers, d_depths, nlayers, order, npix, d_out, d_depth_out, stream);
}
