// smk_step_blend.hip -- fractional time (smk.h: smk_blend_timesteps; DESIGN.md 3b "Fractional time").
// A blended step is a step: the packed voxels of two slots blended field by field into a third, then the brick summaries
// of the result, as after an upload.  The arithmetic is smk.h's: u = 1 - w once on the host, r = (u * x) + (w * y) in fp32
// with one rounding per operation (two products, one sum: the build's -ffp-contract=off, restated below), a float field
// stores r, an integer field min((int)(r + 0.5f), top).
#pragma clang fp contract(off)

#include <algorithm>

#include "smk_internal.h"

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
  const int ka = step_a < 0 ? -1 : smk_step_slot(c, step_a), kb = step_b < 0 ? -1 : smk_step_slot(c, step_b);
  if (ka < 0) FAIL(c, "%s: time step %d (a) is not cached", who, step_a);
  if (kb < 0) FAIL(c, "%s: time step %d (b) is not cached", who, step_b);
  if (step_out < 0) FAIL(c, "%s: output time step %d: ids are >= 0", who, step_out);
  if (step_out == step_a || step_out == step_b)
    FAIL(c, "%s: output time step %d is also a source: the blend has no in-place form", who, step_out);
  if (!(w >= 0.0f && w <= 1.0f)) FAIL(c, "%s: weight %g is not in [0, 1] (no extrapolation)", who, (double)w);
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  const float u = 1.0f - w;
  // the sources, the current step and the output are 3 or 4 slots (one less where a and b are the same step)
  if (smk_step_produce(c, who, step_out, ka, kb, s, [&](TimeStep &T, const TimeStep *A, const TimeStep *B) -> int {
        const size_t nst = (size_t)c->D[0] * c->D[1] * c->D[2];
        // the stored box in 16-byte units (a whole number of them: smk_packed.h); the 16 bytes behind the box are not touched
        const size_t units = c->vox_bytes / 16;
        if (c->dtype == SMK_U8) HIPCHK(c, launch_blend<SMK_U8>(A->vox, B->vox, T.vox, units, u, w, s));
        else if (c->dtype == SMK_U16) HIPCHK(c, launch_blend<SMK_U16>(A->vox, B->vox, T.vox, units, u, w, s));
        else if (c->nelts <= 3) HIPCHK(c, launch_blend<TB_F32N>(A->vox, B->vox, T.vox, units, u, w, s));
        else HIPCHK(c, launch_blend<TB_F32C>(A->vox, B->vox, T.vox, units, u, w, s));
        if (smk_step_nrm_bytes(c)) {
          // the separate normals of four-channel f32, a word per voxel, in the byte form: the whole units, then the words that
          // are left when the voxel count (odd sizes are allowed for f32) is no multiple of four
          HIPCHK(c, launch_blend<SMK_U8>(A->nrm, B->nrm, T.nrm, nst / 4, u, w, s));
          if (nst % 4) {
            const size_t done = nst / 4 * 4;
            hipLaunchKernelGGL(smk_k_blend_words, dim3(1), dim3(64), 0, s, A->nrm + done, B->nrm + done, T.nrm + done, (int)(nst % 4), u, w);
            HIPCHK(c, hipGetLastError());
          }
        }
        return 0;
      }))
    return 1;
  ++c->tblend_count;
  return 0;
}
