// smk_step_hist.hip -- the joint histogram and the data probe of a RESIDENT time step, read from its packed voxels
// (smk.h: smk_hist2d_step_device, smk_hist2d_step, smk_probe_step; DESIGN.md 3b "Histogram and probe of a step").
//
// MetaVolume::hist2D (MetaVolume.cpp:1650-1688) and TFWidgetRen::drawProbe's data half (TFWidgetRen1.cpp:309-595) read
// the host's [z][y][x][nelts] array.  A step that came from a device buffer, a blended step, a shard's region and 16-bit
// voxels have no such array: what the context owns is the packed voxels of a ring slot (TimeStep::vox), so these entries
// read those.  smk_prep.hip's histogram kernels stay what they are for raw arrays; this file holds the packed-layout family.
// The packed layouts, the stored box and the region's rows: smk_packed.h.  The histogram counts the region [g0, g1) alone.
#include <string.h>

#include <algorithm>
#include <vector>

#include "smk_internal.h"
#include "smk_prep_device.h"

namespace {

constexpr int SH_PER = 4;  // units a lane loads before it bins them (a chunk's last turn is a partial one)

struct StepHistParams {
  const uint4 *vox;  // the slot's packed voxels
  unsigned *bins;    // [65536] global counts
  StepRows R;
};

// the key b1 * 256 + b0 of an 8-byte voxel's first word
template <int L>
__device__ __forceinline__ unsigned sh_key8(unsigned w) {
  if (L == SMK_U8) return w & 0xffffu;  // the two bytes are the bins
  return smk_u16_bin(smk_vox8_c0<SMK_U16>(w)) | smk_u16_bin(smk_vox8_c1<SMK_U16>(w)) << 8;
}

// a lane's SH_PER units of the turn that starts at unit k of the chunk that starts at C, and their columns
__device__ __forceinline__ void sh_load(const StepHistParams &P, unsigned k, unsigned lim, const StepOrigin &C, uint4 (&x)[SH_PER],
                                        unsigned (&col)[SH_PER]) {
#pragma unroll
  for (int j = 0; j < SH_PER; ++j) {
    const unsigned i = k + (unsigned)j * 1024 + threadIdx.x;
    col[j] = 0;
    x[j] = make_uint4(0, 0, 0, 0);
    if (i < lim) {
      unsigned q;
      x[j] = P.vox[step_unit(P.R, C, i, col[j], q)];
    }
  }
}

// All 65536 bins as 16-bit LDS counters, flushed to the global bins after a chunk of at most HIST_CHUNK voxels.  A chunk is a
// run of consecutive units of the region's rows; its first unit's row and column are found once per chunk, a lane's from there.
template <int L>
__global__ __launch_bounds__(1024) void smk_k_step_hist(const StepHistParams P) {
  extern __shared__ unsigned h16[];  // 32768 words = 65536 halves
  constexpr unsigned CH = L == SMK_F32 ? HIST_CHUNK : HIST_CHUNK / 2;  // units per chunk
  const unsigned long long nchunks = (P.R.units + CH - 1) / CH;
  for (unsigned long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    hist_lds_zero(h16);
    const unsigned long long base = chunk * CH;
    const unsigned lim = P.R.units - base < CH ? (unsigned)(P.R.units - base) : CH;
    const StepOrigin C = step_chunk_origin(P.R, base);
    // a turn = SH_PER units per lane; the next turn's loads are issued before this turn's units are binned
    uint4 x[SH_PER], xn[SH_PER];
    unsigned col[SH_PER], coln[SH_PER];
    sh_load(P, 0, lim, C, x, col);
    for (unsigned k = 0; k < lim; k += 1024 * SH_PER) {
      if (k + 1024 * SH_PER < lim) sh_load(P, k + 1024 * SH_PER, lim, C, xn, coln);
#pragma unroll
      for (int j = 0; j < SH_PER; ++j) {
        const bool ok = k + (unsigned)j * 1024 + threadIdx.x < lim;
        if (L == SMK_F32) {
          hist_lds_count(h16, ok, ok ? hist_bin_f32(__uint_as_float(x[j].x)) | hist_bin_f32(__uint_as_float(x[j].y)) << 8 : 0u);
        } else {
          hist_lds_count(h16, ok && !step_low_masked(P.R, col[j]), ok ? sh_key8<L>(x[j].x) : 0u);
          hist_lds_count(h16, ok && !step_high_masked(P.R, col[j]), ok ? sh_key8<L>(x[j].z) : 0u);
        }
      }
#pragma unroll
      for (int j = 0; j < SH_PER; ++j) {
        x[j] = xn[j];
        col[j] = coln[j];
      }
    }
    hist_lds_flush(h16, P.bins);
  }
}

template <int L>
hipError_t launch_step_hist(const StepHistParams &P, int device, hipStream_t s) {
  static bool attr[64] = {};  // per device
  if (const hipError_t e = hist_lds_allow((const void *)smk_k_step_hist<L>, device, attr); e != hipSuccess) return e;
  const unsigned long long ch = L == SMK_F32 ? HIST_CHUNK : HIST_CHUNK / 2, nchunks = (P.R.units + ch - 1) / ch;
  const unsigned blocks = (unsigned)std::min<unsigned long long>(nchunks, 256);  // one workgroup per CU is resident (its LDS): they stride
  hipLaunchKernelGGL(smk_k_step_hist<L>, dim3(blocks), dim3(1024), HIST_LDS_BYTES, s, P);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the probe's fetch

struct StepProbeParams {
  const void *vox;
  const uint32_t *nrm;  // the separate normals of four-channel f32, or null
  int O[3], D[3];
  int vlo[3], vhi[3];   // the step's valid box, global voxels: the stored box cut at the volume, less the rim a sharded stencil producer left
  int dtype, nelts;
  const int *cells;     // [n][3]
  int n;
  float *raw;           // [n][8][4]
  uint32_t *nrmw;       // [n][8] n0 | n1 << 8 | n2 << 16
  int *ok;              // [n]
};

// One lane per corner (i * 4 + j * 2 + k: i along z, j along y, k along x).  A cell is answered when its eight corners lie
// in the step's valid box (TimeStep::vlo, vhi: inside the volume and the stored box, whose pad column is outside the volume,
// and off the rim of a sharded stencil producer's result); otherwise its outputs are zeros.
__global__ __launch_bounds__(256) void smk_k_step_probe(const StepProbeParams P) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)P.n * 8) return;
  const int cell = (int)(t >> 3), corner = (int)(t & 7);
  const int d[3] = {corner & 1, (corner >> 1) & 1, corner >> 2};
  bool ok = true;
  size_t o = 0;
  for (int a = 2; a >= 0; --a) {
    const int lo = P.cells[cell * 3 + a];
    ok = ok && lo >= P.vlo[a] && lo < P.vhi[a] - 1;  // (lo + 1 <= vhi - 1, without the overflow of lo + 1)
    o = o * (size_t)P.D[a] + (size_t)(ok ? lo + d[a] - P.O[a] : 0);
  }
  uint32_t r[4] = {0, 0, 0, 0}, nb = 0;
  if (ok) {
    if (P.dtype == SMK_F32) {
      const uint4 v = ((const uint4 *)P.vox)[o];
      r[0] = v.x; r[1] = v.y; r[2] = v.z;
      if (P.nelts == 4) r[3] = v.w;
      nb = smk_nrm_bits(smk_f32_nrm_word(v, P.nelts, P.nrm ? P.nrm[o] : SMK_NRM_NONE));
    } else {
      const uint2 v = ((const uint2 *)P.vox)[o];
      nb = smk_nrm_bits(v.y);
      if (P.dtype == SMK_U8) {
        for (int e = 0; e < 4; ++e) r[e] = __float_as_uint((float)smk_u8_ch(v.x, e));
      } else {
        r[0] = __float_as_uint((float)smk_vox8_c0<SMK_U16>(v.x));
        r[1] = __float_as_uint((float)smk_vox8_c1<SMK_U16>(v.x));
        r[2] = __float_as_uint((float)smk_u16_q2(v.y));
        r[3] = __float_as_uint(0.f);
      }
    }
  }
  ((uint4 *)P.raw)[t] = make_uint4(r[0], r[1], r[2], r[3]);  // (floats moved as bits: an f32 voxel comes back bit for bit)
  P.nrmw[t] = nb;
  if (corner == 0) P.ok[cell] = ok ? 1 : 0;
}

int hist_enqueue(smk_ctx *c, const char *who, int timestep, void *d_counts, hipStream_t s) {
  int k = -1;
  if (step_slot(c, who, timestep, &k)) return 1;
  if (c->nelts < 2) FAIL(c, "%s: sorry this type of histogram is not implemented (needs value and gradient channels)", who);
  if (!d_counts) FAIL(c, "%s: d_counts is NULL", who);
  TimeStep &T = c->ts[(size_t)k];
  StepHistParams P;
  P.vox = (const uint4 *)T.vox;
  P.bins = (unsigned *)d_counts;
  P.R = smk_step_rows(c);
  if (!P.R.units) FAIL(c, "%s: this context's region is empty", who);
  if ((unsigned long long)P.R.upr + HIST_CHUNK > 0xffffffffull) FAIL(c, "%s: rows of %u voxels are too long", who, P.R.nx);
  // behind the step's writer; what overwrites the slot later waits for this read (smk_timesteps.hip)
  return smk_step_read(c, k, -1, s, [&]() -> int {
    HIPCHK(c, hipMemsetAsync(d_counts, 0, 65536 * sizeof(unsigned), s));
    HIPCHK(c, c->dtype == SMK_U8    ? launch_step_hist<SMK_U8>(P, c->device, s)
              : c->dtype == SMK_U16 ? launch_step_hist<SMK_U16>(P, c->device, s) : launch_step_hist<SMK_F32>(P, c->device, s));
    return 0;
  });
}

}  // namespace

extern "C" int smk_hist2d_step_device(smk_ctx *c, int timestep, void *d_counts, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  return hist_enqueue(c, "smk_hist2d_step_device", timestep, d_counts, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_hist2d_step(smk_ctx *c, int timestep, unsigned *counts, unsigned char *hist) {
  if (!c) return 1;
  const char *who = "smk_hist2d_step";
  HIPCHK(c, hipSetDevice(c->device));
  if (!counts && !hist) FAIL(c, "%s: neither counts nor hist is given", who);
  unsigned *d_bins = nullptr;
  HIPCHK(c, hipMalloc((void **)&d_bins, 65536 * sizeof(unsigned)));
  std::vector<unsigned> mine;
  if (!counts) {
    mine.resize(65536);
    counts = mine.data();
  }
  int rc = hist_enqueue(c, who, timestep, d_bins, c->stream);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(counts, d_bins, 65536 * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      c->err = std::string(who) + ": " + hipGetErrorString(e);
      rc = 1;
    }
  }
  (void)hipFree(d_bins);
  if (rc) return 1;
  if (hist) smk_hist2d_finish(counts, hist);
  return 0;
}

extern "C" int smk_probe_step(smk_ctx *c, int timestep, const int *cells, int n, float *raw_out, unsigned char *nrm_out, int *ok_out) {
  if (!c) return 1;
  const char *who = "smk_probe_step";
  HIPCHK(c, hipSetDevice(c->device));
  int k = -1;
  if (step_slot(c, who, timestep, &k)) return 1;
  if (n < 1 || n > 65536) FAIL(c, "%s: %d cells: 1 to 65536 per call", who, n);
  if (!cells || !raw_out || !ok_out) FAIL(c, "%s: cells, raw_out and ok_out must be given", who);
  TimeStep &T = c->ts[(size_t)k];
  // one device buffer: the cells, then the three outputs
  const size_t nc = (size_t)n, b_cells = nc * 3 * sizeof(int), b_raw = nc * 32 * sizeof(float), b_nrm = nc * 8 * sizeof(uint32_t),
               b_ok = nc * sizeof(int), o_raw = (b_cells + 15) / 16 * 16, o_nrm = o_raw + b_raw, o_ok = o_nrm + b_nrm;
  char *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, o_ok + b_ok));
  StepProbeParams P;
  P.vox = T.vox;
  P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
  for (int a = 0; a < 3; ++a) {
    P.O[a] = c->O[a];
    P.D[a] = c->D[a];
    P.vlo[a] = T.vlo[a];
    P.vhi[a] = T.vhi[a];
  }
  P.dtype = c->dtype;
  P.nelts = c->nelts;
  P.cells = (const int *)d;
  P.n = n;
  P.raw = (float *)(d + o_raw);
  P.nrmw = (uint32_t *)(d + o_nrm);
  P.ok = (int *)(d + o_ok);
  std::vector<uint32_t> nw(nrm_out ? nc * 8 : 0);
  const hipStream_t s = c->stream;
  hipError_t e = hipMemcpyAsync(d, cells, b_cells, hipMemcpyHostToDevice, s);
  int rc = e != hipSuccess;
  if (!rc) rc = smk_step_read_begin(c, k, s);
  if (!rc) {
    hipLaunchKernelGGL(smk_k_step_probe, dim3((unsigned)((nc * 8 + 255) / 256)), dim3(256), 0, s, P);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(raw_out, P.raw, b_raw, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && nrm_out) e = hipMemcpyAsync(nw.data(), P.nrmw, b_nrm, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(ok_out, P.ok, b_ok, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (synchronous: nothing of this read is left for the slot's next writer)
    rc = e != hipSuccess;
  }
  if (rc && e != hipSuccess) c->err = std::string(who) + ": " + hipGetErrorString(e);
  (void)hipFree(d);
  if (rc) return 1;
  if (nrm_out)
    for (size_t i = 0; i < nc * 8; ++i) {
      const bool ok = ok_out[i >> 3] != 0;
      for (int a = 0; a < 3; ++a) nrm_out[i * 3 + a] = ok ? (unsigned char)(nw[i] >> (8 * a)) : 0;
    }
  return 0;
}
