// smk_step_read.hip -- a RESIDENT time step read back as the caller's arrays: raw voxels [z][y][x][nelts] and normals
// [z][y][x][3] from the packed voxels of a ring slot (smk.h: smk_get_timestep_box, smk_download_timestep_device,
// smk_download_timestep; DESIGN.md 3b "Reading a step back").  The inverse of smk_k_pack (smk_api.hip).
//
// MetaVolume::writeAll / Volume::writeVol (MetaVolume.cpp:99-126, 963-1000) write the host's currentData / currentGrad.  A
// step that came from a device buffer, a blended step and a shard's region have neither: what the context owns is the slot's
// packed voxels (TimeStep::vox, and TimeStep::nrm for four-channel f32), so these entries read those.
//
// Reads: the region's rows in whole 16-byte units (smk_packed.h, with the packed layouts and the stored box).
// Writes.  The output is dense, so the region's voxels in row order ARE the output in address order: a chunk of consecutive
// units is one run of output bytes, which starts and ends on any byte (9 voxels x 3 bytes are a 27-byte row).  A workgroup
// puts its chunk's bytes into LDS at the phase the run has in its 16-byte line of the OUTPUT, then writes whole lines as
// 16-byte stores and the two ragged ends byte by byte: exactly the bytes of the two arrays are written, none beside them.
#include <algorithm>

#include "smk_internal.h"

namespace {

constexpr int SR_PER = 4;                          // units a lane loads per chunk
constexpr unsigned SR_LANES = 256;
constexpr unsigned SR_CHUNK = SR_LANES * SR_PER;   // units per chunk: a wave's load instruction covers 1 KiB
constexpr unsigned SR_MAX_BLOCKS = 2048;           // 8 workgroups for each of 256 CUs: they stride over the chunks

struct StepReadParams {
  const uint4 *vox;     // the slot's packed voxels
  const uint32_t *nrm;  // the separate normals of four-channel f32, or null
  unsigned char *data;  // [nvox][nelts] elements of the step's type
  unsigned char *grad;  // [nvox][3] bytes, or null
  StepRows R;
  unsigned nelts;
};

// a chunk of consecutive units of the region's rows: where it starts, its length (0 past the last chunk), the first voxel x0
// of the run it starts in its row, and the output voxel that is (the end of the output for a chunk past the last)
struct SrChunk {
  StepOrigin o;
  unsigned lim, x0;
  unsigned long long v0;
};

template <int L>
__device__ __forceinline__ SrChunk sr_chunk(const StepReadParams &P, unsigned long long chunk) {
  const unsigned long long base = chunk * SR_CHUNK;
  SrChunk C = {{0, 0, 0, 0}, 0, 0, P.R.nvox};
  if (base >= P.R.units) return C;
  C.lim = P.R.units - base < SR_CHUNK ? (unsigned)(P.R.units - base) : SR_CHUNK;
  C.o = step_chunk_origin(P.R, base);
  C.x0 = L == SMK_F32 ? C.o.u0 : (C.o.u0 ? 2 * C.o.u0 - P.R.head : 0);
  C.v0 = C.o.row0 * P.R.nx + C.x0;
  return C;
}

// a lane's SR_PER units of chunk C, their columns, and the chunk-local output index of each unit's (low) voxel: -1 for the
// masked low voxel of a row's first unit.  n: the normal word of a four-channel f32 voxel
template <int L>
__device__ __forceinline__ void sr_load(const StepReadParams &P, const SrChunk &C, uint4 (&x)[SR_PER], uint32_t (&n)[SR_PER],
                                        unsigned (&col)[SR_PER], int (&lv)[SR_PER]) {
#pragma unroll
  for (int j = 0; j < SR_PER; ++j) {
    const unsigned i = (unsigned)j * SR_LANES + threadIdx.x;
    x[j] = make_uint4(0, 0, 0, 0);
    n[j] = SMK_NRM_NONE;
    col[j] = 0;
    lv[j] = 0;
    if (i < C.lim) {
      unsigned q;
      const unsigned long long o = step_unit(P.R, C.o, i, col[j], q);
      x[j] = P.vox[o];
      if (L == SMK_F32) {
        if (P.nrm) n[j] = P.nrm[o];  // (a unit is a voxel: the same index)
        lv[j] = (int)(q * P.R.nx + col[j] - C.x0);
      } else {
        lv[j] = (int)(q * P.R.nx + 2 * col[j] - C.x0) - (int)P.R.head;
      }
    }
  }
}

typedef uint32_t __attribute__((may_alias)) sr_u32;
typedef unsigned short __attribute__((may_alias)) sr_u16;
typedef uint4 __attribute__((may_alias)) sr_u128;

// one 8-byte voxel {w0, w1} into the staged run: its channels at d, its three normal bytes at g (null: none wanted)
template <int L>
__device__ __forceinline__ void sr_put8(unsigned char *d, unsigned char *g, uint32_t w0, uint32_t w1, unsigned nelts) {
  if (L == SMK_U8) {
#pragma unroll
    for (unsigned e = 0; e < 4; ++e)
      if (e < nelts) d[e] = (unsigned char)smk_u8_ch(w0, (int)e);
  } else {
    sr_u16 *h = (sr_u16 *)d;  // (the run's phase is even: d_data has the element's alignment)
    h[0] = (unsigned short)smk_vox8_c0<SMK_U16>(w0);
    if (nelts > 1) h[1] = (unsigned short)smk_vox8_c1<SMK_U16>(w0);
    if (nelts > 2) h[2] = (unsigned short)smk_q8_expand(smk_u16_q2(w1));  // the stored 8-bit field q as the 16-bit value 257 q
  }
  if (g) smk_nrm_bytes(w1, g);
}

// the staged run lds[ph, ph + nb) to out[0, nb): LDS byte k is output byte k - ph, and out - ph is 16-byte aligned, so
// the whole 16-byte lines of the run go out as one store each; the (at most two) ragged lines byte by byte
__device__ __forceinline__ void sr_flush(unsigned char *out, const unsigned char *lds, unsigned ph, unsigned nb) {
  unsigned char *line0 = out - ph;
  const unsigned end = ph + nb, n16 = (end + 15) / 16;
  for (unsigned i = threadIdx.x; i < n16; i += SR_LANES) {
    const unsigned lo = 16 * i;
    if (lo >= ph && lo + 16 <= end) {
      ((uint4 *)line0)[i] = ((const sr_u128 *)lds)[i];
    } else {
      const unsigned b = lo > ph ? lo : ph, e = lo + 16 < end ? lo + 16 : end;
      for (unsigned k = b; k < e; ++k) line0[k] = lds[k];
    }
  }
}

// voxels a chunk can hold, and the bytes of its two staged runs (+ 16: the run's phase in its first line)
template <int L>
struct SrLds {
  static constexpr unsigned VOX = L == SMK_F32 ? SR_CHUNK : 2 * SR_CHUNK;
  static constexpr unsigned DATA = VOX * (L == SMK_U16 ? 3 : 4) * (unsigned)smk_elem_bytes(L) + 16;  // (u16 has up to 3 channels)
  static constexpr unsigned GRAD = VOX * 3 + 16;
};

// One pass over the region's rows.  A workgroup takes chunks of SR_CHUNK consecutive units in turn; the loads of its next
// chunk are issued before the bytes of this one are staged and written.
template <int L>
__global__ __launch_bounds__(256) void smk_k_unpack_step(const StepReadParams P) {
  __shared__ uint4 s_data[SrLds<L>::DATA / 16], s_grad[SrLds<L>::GRAD / 16];
  unsigned char *sd = (unsigned char *)s_data, *sg = (unsigned char *)s_grad;
  const unsigned vb = P.nelts * (unsigned)smk_elem_bytes(L);  // bytes of an output voxel
  const unsigned long long nchunks = (P.R.units + SR_CHUNK - 1) / SR_CHUNK;
  unsigned long long chunk = blockIdx.x;
  if (chunk >= nchunks) return;
  SrChunk C = sr_chunk<L>(P, chunk);
  uint4 x[SR_PER], xn[SR_PER];
  uint32_t n[SR_PER], nn[SR_PER];
  unsigned col[SR_PER], coln[SR_PER];
  int lv[SR_PER], lvn[SR_PER];
  sr_load<L>(P, C, x, n, col, lv);
  for (; chunk < nchunks; chunk += gridDim.x) {
    const SrChunk Cn = sr_chunk<L>(P, chunk + gridDim.x);
    if (Cn.lim) sr_load<L>(P, Cn, xn, nn, coln, lvn);
    // this chunk's run: the output voxels [C.v0, the first voxel of the chunk behind it)
    const unsigned nv = (unsigned)(sr_chunk<L>(P, chunk + 1).v0 - C.v0);
    unsigned char *od = P.data + C.v0 * vb, *og = P.grad ? P.grad + C.v0 * 3 : nullptr;
    const unsigned phd = (unsigned)((uintptr_t)od & 15), phg = (unsigned)((uintptr_t)og & 15);
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) {
      if ((unsigned)j * SR_LANES + threadIdx.x >= C.lim) continue;
      if (L == SMK_F32) {
        sr_u32 *d = (sr_u32 *)(sd + phd + (unsigned)lv[j] * vb);  // (phd is a multiple of 4: d_data is float-aligned)
        d[0] = x[j].x;
        if (P.nelts > 1) d[1] = x[j].y;
        if (P.nelts > 2) d[2] = x[j].z;
        if (P.nelts > 3) d[3] = x[j].w;
        if (og) {
          smk_nrm_bytes(smk_f32_nrm_word(x[j], (int)P.nelts, n[j]), sg + phg + (unsigned)lv[j] * 3);
        }
      } else {
        if (!step_low_masked(P.R, col[j]))
          sr_put8<L>(sd + phd + (unsigned)lv[j] * vb, og ? sg + phg + (unsigned)lv[j] * 3 : nullptr, x[j].x, x[j].y, P.nelts);
        if (!step_high_masked(P.R, col[j]))
          sr_put8<L>(sd + phd + (unsigned)(lv[j] + 1) * vb, og ? sg + phg + (unsigned)(lv[j] + 1) * 3 : nullptr, x[j].z, x[j].w, P.nelts);
      }
    }
    __syncthreads();
    sr_flush(od, sd, phd, nv * vb);
    if (og) sr_flush(og, sg, phg, nv * 3);
    __syncthreads();
    C = Cn;
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) {
      x[j] = xn[j];
      n[j] = nn[j];
      col[j] = coln[j];
      lv[j] = lvn[j];
    }
  }
}

template <int L>
hipError_t launch_unpack(const StepReadParams &P, hipStream_t s) {
  const unsigned long long nchunks = (P.R.units + SR_CHUNK - 1) / SR_CHUNK;
  const unsigned blocks = (unsigned)std::min<unsigned long long>(nchunks, SR_MAX_BLOCKS);
  hipLaunchKernelGGL(smk_k_unpack_step<L>, dim3(blocks), dim3(SR_LANES), 0, s, P);
  return hipGetLastError();
}

int read_enqueue(smk_ctx *c, const char *who, int k, void *d_data, void *d_grad, hipStream_t s) {
  TimeStep &T = c->ts[(size_t)k];
  const size_t eb = smk_elem_bytes(c->dtype);
  if ((uintptr_t)d_data % eb) FAIL(c, "%s: d_data is not aligned to its %zu-byte elements", who, eb);
  StepReadParams P;
  P.vox = (const uint4 *)T.vox;
  P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
  P.data = (unsigned char *)d_data;
  P.grad = (unsigned char *)d_grad;
  P.R = smk_step_rows(c);
  P.nelts = (unsigned)c->nelts;
  if (!P.R.units) FAIL(c, "%s: this context's region is empty", who);
  // behind the step's writer; what overwrites the slot later waits for this read (smk_timesteps.hip)
  return smk_step_read(c, k, -1, s, [&]() -> int {
    HIPCHK(c, c->dtype == SMK_U8 ? launch_unpack<SMK_U8>(P, s) : c->dtype == SMK_U16 ? launch_unpack<SMK_U16>(P, s) : launch_unpack<SMK_F32>(P, s));
    return 0;
  });
}

}  // namespace

extern "C" int smk_get_timestep_box(smk_ctx *c, int origin[3], int size[3], int *nelts, smk_dtype *dtype, int *has_normals) {
  if (!c) return 1;
  if (!c->have_volume) FAIL(c, "smk_get_timestep_box: no volume uploaded");
  for (int a = 0; a < 3; ++a) {
    if (origin) origin[a] = c->g0[a];
    if (size) size[a] = c->g1[a] - c->g0[a];
  }
  if (nelts) *nelts = c->nelts;
  if (dtype) *dtype = (smk_dtype)c->dtype;
  if (has_normals) *has_normals = c->have_normals ? 1 : 0;
  return 0;
}

extern "C" int smk_download_timestep_device(smk_ctx *c, int timestep, void *d_data, void *d_grad, void *stream) {
  if (!c) return 1;
  const char *who = "smk_download_timestep_device";
  HIPCHK(c, hipSetDevice(c->device));
  int k = -1;
  if (step_slot(c, who, timestep, &k)) return 1;
  if (!d_data) FAIL(c, "%s: d_data is NULL", who);
  return read_enqueue(c, who, k, d_data, d_grad, stream ? (hipStream_t)stream : c->stream);
}

extern "C" int smk_download_timestep(smk_ctx *c, int timestep, void *data, unsigned char *grad) {
  if (!c) return 1;
  const char *who = "smk_download_timestep";
  HIPCHK(c, hipSetDevice(c->device));
  int k = -1;
  if (step_slot(c, who, timestep, &k)) return 1;
  if (!data) FAIL(c, "%s: data is NULL", who);
  // one staging buffer of the box's size: the voxels, then (from a 16-byte boundary) the normals
  const size_t nvox = (size_t)(c->g1[0] - c->g0[0]) * (size_t)(c->g1[1] - c->g0[1]) * (size_t)(c->g1[2] - c->g0[2]);
  const size_t b_data = nvox * (size_t)c->nelts * smk_elem_bytes(c->dtype), b_grad = grad ? nvox * 3 : 0, o_grad = (b_data + 15) / 16 * 16;
  const size_t need = o_grad + b_grad;
  if (!need) FAIL(c, "%s: this context's region is empty", who);
  size_t fr = 0, tot = 0;
  HIPCHK(c, hipMemGetInfo(&fr, &tot));
  if (need > fr) FAIL(c, "%s: the staging buffers of the box do not fit: %zu bytes needed, %zu free", who, need, fr);
  char *d = nullptr;
  HIPCHK(c, hipMalloc((void **)&d, need));
  const hipStream_t s = c->stream;
  int rc = read_enqueue(c, who, k, d, grad ? d + o_grad : nullptr, s);
  if (!rc) {
    hipError_t e = hipMemcpyAsync(data, d, b_data, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && grad) e = hipMemcpyAsync(grad, d + o_grad, b_grad, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      c->err = std::string(who) + ": " + hipGetErrorString(e);
      rc = 1;
    }
  }
  (void)hipFree(d);
  return rc;
}
