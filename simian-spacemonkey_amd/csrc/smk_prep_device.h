// smk_prep_device.h -- the device arithmetic of the data-preparation kernels (smk_prep.hip), shared with the kernels that
// derive or merge a resident time step inside the ring (smk_step_derive.hip, smk_step_merge.hip): one statement of every
// expression, so that all give the same bits.  Plain fp32, doubles inside affine_d, one rounding per operation in the order written (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

// order-preserving float <-> int map so min/max can use integer atomics
__device__ __forceinline__ int f2o(float f) {
  int i = __float_as_int(f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float o2f(int i) {
  int j = i >= 0 ? i : i ^ 0x7fffffff;
#ifdef __HIP_DEVICE_COMPILE__
  return __int_as_float(j);
#else
  float f;
  memcpy(&f, &j, 4);
  return f;
#endif
}

struct VghStats {  // ordered-int encoded
  int dmin, dmax, gmin, gmax, hmin, hmax;
};

// Where a kernel that makes a step inside the ring reads from, as its SRC template argument: dense arrays of a type (their
// smk_dtype, 0..2), or the packed voxels of a slot of that type
enum { SRC_PK_U8 = 3, SRC_PK_U16 = 4, SRC_PK_F32 = 5 };

#define ORD_POS_INF 0x7f800000
#define ORD_NEG_INF ((int)0x807fffff)  // f2o(-inf) = 0xff800000 ^ 0x7fffffff

__device__ __forceinline__ bool is_border(int sx, int sy, int sz, int i, int j, int k) {
  return (k < 1) || (k > sx - 2) || (j < 1) || (j > sy - 2) || (i < 1) || (i > sz - 2);
}

// gradient magnitude + second derivative along the gradient (genVGH/main.cpp:110-146) from the un-normalised central
// differences g of a voxel and those of its six neighbours (zero where the neighbour lies on the 1-voxel border)
__device__ __forceinline__ void gh_from_grads(const float g[3], const float xp[3], const float xm[3], const float yp[3],
                                              const float ym[3], const float zp[3], const float zm[3], int compat, float &gm,
                                              float &hs) {
  gm = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  float h[9];
  h[0] = xp[0] - xm[0];
  h[1] = yp[0] - ym[0];
  h[2] = zp[0] - zm[0];
  h[3] = xp[1] - xm[1];
  h[4] = yp[1] - ym[1];
  h[5] = zp[1] - zm[1];
  h[6] = xp[2] - xm[2];
  h[7] = yp[2] - ym[2];
  h[8] = zp[2] - zm[2];
  float tg[3] = {g[0] / gm, g[1] / gm, g[2] / gm};
  float tv0 = tg[0] * h[0] + tg[1] * h[1] + tg[2] * h[2];
  // the reference drops h[4] here (genVGH/main.cpp:135-137); compat keeps the typo
  float tv1 = compat ? tg[0] * h[3] + tg[1] + tg[2] * h[5] : tg[0] * h[3] + tg[1] * h[4] + tg[2] * h[5];
  float tv2 = tg[0] * h[6] + tg[1] * h[7] + tg[2] * h[8];
  hs = tg[0] * tv0 + tg[1] * tv1 + tg[2] * tv2;
}

__device__ __forceinline__ int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}

// a thread's running extremes of the interior voxels it visits, and their way into the device words
struct VghRunning {
  int dmin = ORD_POS_INF, dmax = ORD_NEG_INF, gmin = ORD_POS_INF, gmax = ORD_NEG_INF, hmin = ORD_POS_INF, hmax = ORD_NEG_INF;
  __device__ __forceinline__ void take(float dv, float gm, float hs) {
    dmin = min(dmin, f2o(dv));
    dmax = max(dmax, f2o(dv));
    gmin = min(gmin, f2o(gm));
    gmax = max(gmax, f2o(gm));
    if (hs == hs) {  // NaN (zero gradient) never wins the reference's MAX/MIN macros
      hmin = min(hmin, f2o(hs));
      hmax = max(hmax, f2o(hs));
    }
  }
  // wave reduction, then one ordered-int atomic per wave and extreme (every lane of the wave calls this)
  __device__ __forceinline__ void publish(VghStats *st) {
    dmin = wave_min(dmin);
    dmax = wave_max(dmax);
    gmin = wave_min(gmin);
    gmax = wave_max(gmax);
    hmin = wave_min(hmin);
    hmax = wave_max(hmax);
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&st->dmin, dmin);
      atomicMax(&st->dmax, dmax);
      atomicMin(&st->gmin, gmin);
      atomicMax(&st->gmax, gmax);
      atomicMin(&st->hmin, hmin);
      atomicMax(&st->hmax, hmax);
    }
  }
};

__device__ __forceinline__ double affine_d(double i, double x, double I, double o, double O) {
  return ((O) - (o)) * ((x) - (i)) / ((I) - (i)) + (o);
}

// (unsigned char) cast as x86 does it: truncate through int32, low byte; NaN/out of range -> 0
__device__ __forceinline__ unsigned char uc_cast(double x) {
  if (!(x > -2147483649.0 && x < 2147483648.0)) return 0;
  return (unsigned char)((int)x & 0xff);
}

// makeVGH's scaling of an interior voxel (genVGH/main.cpp:164-175): the bytes q and the floats f of V, G and H
__device__ __forceinline__ void vgh_scale(float dv, float gm, float hs, float dmin, float dmax, float gmmin, float gmmax,
                                          float hmin, float hmax, unsigned char q[3], float f[3]) {
  double vq = affine_d(dmin, dv, dmax, 0, 255);
  double gq = affine_d(gmmin, gm, gmmax, 0, 255);
  double hq;
  if (hs < 0) {
    float th = (float)affine_d(hmin, hs, 0, 0, 1);
    hq = affine_d(0, th, 1, 0, 255 / 3);
  } else {
    float th = (float)affine_d(0, hs, hmax, 0, 1);
    hq = affine_d(0, th, 1, 255 / 3, 255 / 3 * 2);
  }
  q[0] = uc_cast(vq);
  q[1] = uc_cast(gq);
  q[2] = uc_cast(hq);
  f[0] = (float)(vq / 255.0);
  f[1] = (float)(gq / 255.0);
  f[2] = (hq == hq) ? (float)(hq / 255.0) : 0.0f;
}

// smk_quantize_u16_device (smk.h): t = v * 65535 (one fp32 multiply); NaN or t < 0 -> 0, t >= 65535 -> 65535, else
// (uint16)(int)(t + 0.5f) -- one fp32 add, then truncation
__device__ __forceinline__ unsigned short quant_u16(float v) {
  const float t = v * 65535.0f;
  if (!(t >= 0.0f)) return 0;
  if (t >= 65535.0f) return 65535;
  return (unsigned short)(int)(t + 0.5f);
}

// scalebiasN (VectorMath.h:1133-1148) with the +1 -> 255 clamp
__device__ __forceinline__ void nrm_store(float g[3], unsigned char *out) {
  float len = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
  if (len > 0) {
    g[0] /= len;
    g[1] /= len;
    g[2] /= len;
  }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    float s = g[e] * 128 + 128;
    out[e] = s >= 255.0f ? 255 : (unsigned char)((int)s & 0xff);
  }
}

__device__ __forceinline__ bool finite3(const float g[3]) {
  return __builtin_isfinite(g[0]) && __builtin_isfinite(g[1]) && __builtin_isfinite(g[2]);
}

// nrm_store behind the float rule: a gradient with a component that is not finite is stored as the zero vector
__device__ __forceinline__ void nrm_store_f32(float g[3], unsigned char *out) {
  if (!finite3(g)) {
    out[0] = out[1] = out[2] = 128;
    return;
  }
  nrm_store(g, out);
}

// The multi-field merge (MetaVolume::mergeMV with addG; smk_prep.hip "multi-field merge", smk_step_merge.hip).  The summed
// gradient starts at merge_grad_zero and takes merge_grad_add once per field, fields ascending: one fp32 subtraction and one
// add per field and axis (byte and 16-bit differences and their sums are exact in float).  It stays zero on the 1-voxel border
__device__ __forceinline__ void merge_grad_zero(float g[3]) { g[0] = g[1] = g[2] = 0.f; }
__device__ __forceinline__ void merge_grad_add(float g[3], float xp, float xm, float yp, float ym, float zp, float zm) {
  g[0] += xp - xm;
  g[1] += yp - ym;
  g[2] += zp - zm;
}
__device__ __forceinline__ float merge_mag(const float g[3]) { return sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]); }

// a thread's running maximum of the magnitudes starts at MERGE_MAX_SEED = f2o(0.0f): magnitudes are >= 0.  The u8 merge
// counts every magnitude, the float merge the finite ones
constexpr int MERGE_MAX_SEED = 0;
__device__ __forceinline__ int merge_max_take(int m, float mag) { return max(m, f2o(mag)); }
__device__ __forceinline__ int merge_max_take_f32(int m, float mag) { return __builtin_isfinite(mag) ? max(m, f2o(mag)) : m; }

// GMag's byte (VectorMath.h:1010-1030), (uchar)(mag/max*255.0): float quotient, double product, the cast as uc_cast
__device__ __forceinline__ unsigned char merge_gmag_u8(float mag, float maxm) { return uc_cast((double)(mag / maxm) * 255.0); }

// the float merge's G: 0 where the magnitude is not finite or the maximum is 0
__device__ __forceinline__ float merge_g_f32(float mag, float maxm) { return (maxm > 0.f && __builtin_isfinite(mag)) ? mag / maxm : 0.f; }

// The merge with H and blurred normals (mergeMV with addH: GMagHess, VectorMath.h:1032-1113, read as makeVGH's
// second-derivative block; smk.h smk_merge_fields_h_device).  hs of an interior voxel is gh_from_grads of the summed gradient
// and the summed gradients of its six neighbours; a border voxel has hs = 0.  The extremes run over the interior voxels: a NaN
// never wins, and in the float pipeline (FLT) nothing that is not finite does
__device__ __forceinline__ bool merge_h_counts(bool flt, float hs) { return flt ? __builtin_isfinite(hs) : hs == hs; }

// the running extremes' words {min H, max H} (ordered-int; seeds ORD_POS_INF, ORD_NEG_INF) behind the reference's +-1e8 seeds,
// taken as std::min / std::max take them
__device__ __forceinline__ void merge_h_extremes(int omin, int omax, float &hmin, float &hmax) {
  const float a = o2f(omin), b = o2f(omax);
  hmin = (100000000.f < a) ? 100000000.f : a;
  hmax = (b < -100000000.f) ? -100000000.f : b;
}

// the H byte and the H float of hs: vgh_scale's third output (the data and the magnitude are not looked at)
__device__ __forceinline__ void merge_h_scale(float hs, float hmin, float hmax, unsigned char &q, float &f) {
  unsigned char q3[3];
  float f3[3];
  vgh_scale(0.f, 0.f, hs, 0.f, 1.f, 0.f, 1.f, hmin, hmax, q3, f3);
  q = q3[2];
  f = f3[2];
}
__device__ __forceinline__ unsigned char merge_h_u8(float hs, float hmin, float hmax) {
  unsigned char q;
  float f;
  merge_h_scale(hs, hmin, hmax, q, f);
  return q;
}
// ... the float pipeline's: 0 where hs is not finite
__device__ __forceinline__ float merge_h_f32(float hs, float hmin, float hmax) {
  unsigned char q;
  float f;
  merge_h_scale(hs, hmin, hmax, q, f);
  return __builtin_isfinite(hs) ? f : 0.f;
}

// The normal's gradient at voxel (i, j, k) = (z, y, x) of an sx x sy x sz volume from grad(si, sj, sk, s[3]), the central
// differences of channel 0 at an INTERIOR voxel (derivative3DVGH, VectorMath.h:874-899; 0 on the border).  Blurred: blurV3D is
// a scatter from every interior voxel to its 27 neighbours in raster order of the SOURCE (VectorMath.h:1232-1266).  Gathering
// the same terms in the same order (source raster order == ascending di, dj, dk) reproduces the float sums bit for bit.
template <class Grad>
__device__ __forceinline__ void nrm_gradient(int blur, int sx, int sy, int sz, int i, int j, int k, float g[3], Grad grad) {
  if (!blur) {
    if (is_border(sx, sy, sz, i, j, k)) g[0] = g[1] = g[2] = 0.f;
    else grad(i, j, k, g);
    return;
  }
  const float w[4] = {1.0f, .3f, .2f, .1f};  // MetaVolume.cpp:1316
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int di = -1; di <= 1; ++di)
    for (int dj = -1; dj <= 1; ++dj)
      for (int dk = -1; dk <= 1; ++dk) {
        int si = i + di, sj = j + dj, sk = k + dk;
        // only interior voxels scatter (loops run 1..n-2)
        if (si < 1 || si > sz - 2 || sj < 1 || sj > sy - 2 || sk < 1 || sk > sx - 2) continue;
        float s[3];
        grad(si, sj, sk, s);
        float ww = w[(di != 0) + (dj != 0) + (dk != 0)];
        a0 = a0 + ww * s[0];
        a1 = a1 + ww * s[1];
        a2 = a2 + ww * s[2];
      }
  const float div = 1.0f + 6 * .3f + 12 * .2f + 8 * .1f;
  g[0] = a0 / div;
  g[1] = a1 / div;
  g[2] = a2 / div;
}

// a float channel's histogram bin: t = v * 255 in fp32; NaN and t < 0 -> 0, t >= 255 -> 255, else (int)t
__device__ __forceinline__ unsigned hist_bin_f32(float v) {
  const float t = v * 255.0f;
  if (!(t >= 0.f)) return 0;
  if (t >= 255.f) return 255;
  return (unsigned)(int)t;
}

// Every workgroup (1024 lanes) keeps ALL 65536 bins as 16-bit counters in 128 KB of dynamic LDS (h16: 32768 words) and flushes
// them to the global 32-bit bins after fewer than 65536 voxels, so no counter can overflow
constexpr int HIST_LDS_BYTES = 128 * 1024;
constexpr int HIST_CHUNK = 61440;  // voxels per flush: below 65536, a multiple of the workgroup size

__device__ __forceinline__ void hist_lds_zero(unsigned *h16) {
  for (int w = threadIdx.x; w < 32768; w += 1024) h16[w] = 0;
  __syncthreads();
}

// every lane of a wave calls this (ok: it has a voxel, key: its bin b1 * 256 + b0): live lanes that all share a key add once
__device__ __forceinline__ void hist_lds_count(unsigned *h16, bool ok, unsigned key) {
  const unsigned long long live = __ballot(ok);
  if (!live) return;
  const unsigned first = __builtin_amdgcn_readlane(key, __builtin_ctzll(live));  // (of the first live lane)
  if (__ballot(ok && key == first) == live) {
    if (ok && (int)(threadIdx.x & 63) == __builtin_ctzll(live))
      atomicAdd(&h16[first >> 1], (unsigned)__builtin_popcountll(live) << ((first & 1) * 16));
  } else if (ok) {
    atomicAdd(&h16[key >> 1], 1u << ((key & 1) * 16));
  }
}

__device__ __forceinline__ void hist_lds_flush(const unsigned *h16, unsigned *bins) {
  __syncthreads();
  for (int w = threadIdx.x; w < 32768; w += 1024) {
    const unsigned v = h16[w];
    if (v & 0xffffu) atomicAdd(&bins[2 * w], v & 0xffffu);
    if (v >> 16) atomicAdd(&bins[2 * w + 1], v >> 16);
  }
  __syncthreads();
}

// the kernel's dynamic LDS raised to HIST_LDS_BYTES, once per device: `done` is that kernel's own flags, one per device
inline hipError_t hist_lds_allow(const void *kernel, int device, bool (&done)[64]) {
  if (device >= 0 && device < 64 && done[device]) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HIST_LDS_BYTES);
  if (e == hipSuccess && device >= 0 && device < 64) done[device] = true;
  return e;
}
