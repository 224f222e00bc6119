// smk_clip_slice.hip -- the clip-plane widget's data slice (smk_set_clip_slice): drawClip + renderSlice of the two live
// renderers (R8kVolRen3D.cpp:763-921, shader createFragClip :3190-3250; NV20VolRen3D.cpp:329-528) as ONE pass over the
// finished volume frame.  The reference draws the quad into the framebuffer before the volume's slices (it ends up behind
// them) or after them (on top); both compose with the frame the ray-marchers return, so one kernel, launched behind
// whichever of them ran, serves both: before  frame = volume + (1 - volume.a) src   (max(volume, src) under GL_MAX),
//                                     after   frame = src + (1 - src.a) volume.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "smk_device.h"

extern "C" int smk_set_clip_slice(smk_ctx *c, int on, const float corners[4][3], float alpha, float dv, smk_clip_look look) {
  if (!c) return 1;
  if (!on) {
    c->clip_slice_on = 0;
    return 0;
  }
  if (!corners) FAIL(c, "smk_set_clip_slice: null corners");
  if ((int)look != SMK_CLIP_LOOK_NV20 && (int)look != SMK_CLIP_LOOK_R8K)
    FAIL(c, "smk_set_clip_slice: bad look %d (SMK_CLIP_LOOK_NV20 = 0 or SMK_CLIP_LOOK_R8K = 1)", (int)look);
  for (int k = 0; k < 4; ++k)
    for (int a = 0; a < 3; ++a)
      if (!isfinite(corners[k][a])) FAIL(c, "smk_set_clip_slice: corner %d is not finite", k);
  if (!isfinite(alpha)) FAIL(c, "smk_set_clip_slice: alpha is not finite");
  if (!isfinite(dv)) FAIL(c, "smk_set_clip_slice: dv is not finite");
  memcpy(c->clip_slice_corners, corners, sizeof c->clip_slice_corners);
  c->clip_slice_alpha = alpha;
  c->clip_slice_dv = dv;
  c->clip_slice_look = (int)look;
  c->clip_slice_on = 1;
  return 0;
}

// The quad as two triangles (0, 1, 2), (0, 2, 3) -- GL_QUADS -- against the ray of a pixel.  A ray is X = E + t D with D
// affine in the pixel centre (x, y) = (i + .5, j + .5) and t its view depth, so Moeller-Trumbore's three numerators are
// affine in (x, y) too:  u = D . (e2 x T) / det,  w = D . (T x e1) / det,  t = e2 . (T x e1) / det,  det = D . (e2 x e1),
// T = E - v0.  The host folds them, in double, into f(x, y) = f[0] + f[1] x + f[2] y: these are the quad's screen-space
// edge functions, and the kernel evaluates them in double so that the coverage of a pixel is decided as a float64
// rasteriser decides it (six fma per triangle, one reciprocal per covered pixel).
struct ClipSliceArg {
  double un[2][3], wn[2][3], det[2][3], tn[2];
  double v0[3], e1[2][3], e2[2][3];  // voxel coordinates (model / fSize * N - 0.5)
  float own_lo[3], own_hi[3];        // the hit points this context draws: its region, lo <= X <= hi (hi: the float below an inner face)
  float alpha;
  int pass;                          // 1 before, 2 after
  int blend_max;
  int x0, y0, x1, y1;                // the quad's screen bounding box (x0, y0 multiples of 16; x1, y1 inclusive)
};

// data texel -> colour: 0 the NV20 final combiner, 1..3 the R8k clip shader over a four-, two-, one-byte texture
enum { CS_NV20 = 0, CS_R8K_4B = 1, CS_R8K_2B = 2, CS_R8K_1B = 3 };

// A thread per pixel of the bounding box, 16 x 16 tiles (a wave covers four rows of 16 float4: 256-byte runs).
template <int DT, int LOOK>
__global__ __launch_bounds__(256) void smk_k_clip_slice(const RenderParams P, const ClipSliceArg Q, float4 *fb) {
  const int i = Q.x0 + (int)blockIdx.x * 16 + (int)(threadIdx.x & 15), j = Q.y0 + (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
  if (i > Q.x1 || j > Q.y1) return;
  const double xs = (double)i + 0.5, ys = (double)j + 0.5;
  bool hit = false;
  double X[3] = {0, 0, 0}, tt = 0;
  for (int t = 0; t < 2 && !hit; ++t) {
    // u >= 0, w >= 0, u + w <= 1, t > 0 decided on the numerators: the host has given them the sign that makes t's
    // numerator positive, so a hit in front of the eye has det > 0 (no division before the test)
    const double det = fma(xs, Q.det[t][1], fma(ys, Q.det[t][2], Q.det[t][0]));
    const double un = fma(xs, Q.un[t][1], fma(ys, Q.un[t][2], Q.un[t][0])), wn = fma(xs, Q.wn[t][1], fma(ys, Q.wn[t][2], Q.wn[t][0]));
    if (!(det > 1e-30) || un < 0.0 || wn < 0.0 || un + wn > det) continue;  // (outside, edge-on, or behind the eye)
    hit = true;
    // 1 / det: the float estimate and one Newton step in double (2^-46: the values need 1e-9, not a rounded quotient)
    double r = (double)__frcp_rn((float)det);
    r = fma(fma(-det, r, 1.0), r, r);
    const double u = un * r, w = wn * r;
    tt = Q.tn[t] * r;
    for (int a = 0; a < 3; ++a) X[a] = Q.v0[a] + u * Q.e1[t][a] + w * Q.e2[t][a];
  }
  if (!hit) return;
  const float xf[3] = {(float)X[0], (float)X[1], (float)X[2]};
  // this context's part of the quad: the hit point, brought onto the volume's box (the quad stands 0.001 off the plane and
  // may leave the box by that much), lies in the context's own region
  for (int a = 0; a < 3; ++a) {
    const float xc = smk_clampf(xf[a], -0.5f, (float)P.N[a] - 0.5f);
    if (xc < Q.own_lo[a] || xc > Q.own_hi[a]) return;
  }
  const size_t o = (size_t)j * P.W + i;
  // depth test on, depth writes off: the marchers' comparison against the marchers' scene depth
  if (P.zscene != nullptr && !((float)tt < smk_scene_depth(P, o))) return;
  int x0, x1, y0, y1, z0, z1;
  float fx, fy, fz;
  smk_lin_clamp(xf[0], P.N[0], x0, x1, fx);
  smk_lin_clamp(xf[1], P.N[1], y0, y1, fy);
  smk_lin_clamp(xf[2], P.N[2], z0, z1, fz);
  // region + halo addressing (a hit point of the own region needs the voxels g0 - 1 .. g1: the halo of one)
  x0 = min(max(x0 - P.O[0], 0), P.D[0] - 1); x1 = min(max(x1 - P.O[0], 0), P.D[0] - 1);
  y0 = min(max(y0 - P.O[1], 0), P.D[1] - 1); y1 = min(max(y1 - P.O[1], 0), P.D[1] - 1);
  z0 = min(max(z0 - P.O[2], 0), P.D[2] - 1); z1 = min(max(z1 - P.O[2], 0), P.D[2] - 1);
  const size_t Dx = P.D[0], Dy = P.D[1];
  const size_t r00 = ((size_t)z0 * Dy + y0) * Dx, r10 = ((size_t)z0 * Dy + y1) * Dx, r01 = ((size_t)z1 * Dy + y0) * Dx,
               r11 = ((size_t)z1 * Dy + y1) * Dx;
  const SmkCorner k000 = smk_load_corner<DT>(P, r00 + x0), k100 = smk_load_corner<DT>(P, r00 + x1);
  const SmkCorner k010 = smk_load_corner<DT>(P, r10 + x0), k110 = smk_load_corner<DT>(P, r10 + x1);
  const SmkCorner k001 = smk_load_corner<DT>(P, r01 + x0), k101 = smk_load_corner<DT>(P, r01 + x1);
  const SmkCorner k011 = smk_load_corner<DT>(P, r11 + x0), k111 = smk_load_corner<DT>(P, r11 + x1);
  const float sc = SmkScale<DT>::s01, sch = SmkScale<DT>::s23;
  const float c0 = smk_sat(SMK_TRI(c0) * sc);
  float4 S;
  if (LOOK == CS_NV20) {
    // final combiner: rgb = tex * constant0.a, alpha = constant0.a (NV20VolRen3D.cpp:426-431)
    const float v = c0 * Q.alpha;
    S = make_float4(v, v, v, Q.alpha);
  } else {
    float r = c0, g = 0.0f, b = c0;
    if (LOOK == CS_R8K_4B) {
      g = smk_sat(SMK_TRI(c1) * sc);
      b = smk_sat(SMK_TRI(c2) * sch);
    } else if (LOOK == CS_R8K_2B) {  // GL_LUMINANCE8_ALPHA8: (L, L, L, A), green <- alpha
      g = smk_sat(SMK_TRI(c1) * sc);
    } else {  // GL_ALPHA8: (0, 0, 0, A), green <- alpha
      r = b = 0.0f;
      g = c0;
    }
    const float a = smk_sat(Q.alpha);
    S = make_float4(smk_sat(r * a), smk_sat(g * a), smk_sat(b * a), a);
  }
  float4 V = fb[o];
  if (Q.pass == 1) {
    if (Q.blend_max) {
      V = make_float4(fmaxf(V.x, S.x), fmaxf(V.y, S.y), fmaxf(V.z, S.z), fmaxf(V.w, S.w));
    } else {
      const float w1 = 1.0f - V.w;
      V = make_float4(__fmaf_rn(w1, S.x, V.x), __fmaf_rn(w1, S.y, V.y), __fmaf_rn(w1, S.z, V.z), __fmaf_rn(w1, S.w, V.w));
    }
  } else {
    const float w1 = 1.0f - S.w;
    V = make_float4(__fmaf_rn(w1, V.x, S.x), __fmaf_rn(w1, V.y, S.y), __fmaf_rn(w1, V.z, S.z), __fmaf_rn(w1, V.w, S.w));
  }
  fb[o] = V;
}

static void cross3(double o[3], const double a[3], const double b[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The pass the reference's drawClip would draw the slice in (R8kVolRen3D.cpp:826-879): its case for oaxis, asked with dv
// (before the volume) and with -dv (after); c0 = corner 0's clamped coordinate on the axis.
static bool clip_case(int oaxis, float d, float c0, float fs) {
  const bool in = c0 > 0.0f && c0 < fs;
  switch (oaxis) {
    case 1: return d < 0 && in;
    case 2: return d > 0;  // (no range test in the reference, :835)
    case 3: return d > 0 && in;
    case 4: return d < 0 && in;
    case 5: return d < 0 && in;
    case 6: return d > 0 && in;
  }
  return false;
}

template <int DT>
static void launch_look(int look, dim3 grid, hipStream_t s, const RenderParams &P, const ClipSliceArg &Q, float4 *fb) {
  switch (look) {
    case CS_NV20: hipLaunchKernelGGL((smk_k_clip_slice<DT, CS_NV20>), grid, dim3(256), 0, s, P, Q, fb); break;
    case CS_R8K_4B: hipLaunchKernelGGL((smk_k_clip_slice<DT, CS_R8K_4B>), grid, dim3(256), 0, s, P, Q, fb); break;
    case CS_R8K_2B: hipLaunchKernelGGL((smk_k_clip_slice<DT, CS_R8K_2B>), grid, dim3(256), 0, s, P, Q, fb); break;
    default: hipLaunchKernelGGL((smk_k_clip_slice<DT, CS_R8K_1B>), grid, dim3(256), 0, s, P, Q, fb); break;
  }
}

int smk_clip_slice_stage(smk_ctx *c, const RenderParams &P, hipStream_t s) {
  c->clip_slice_pass = 0;
  if (!c->clip_slice_on || c->clip_axis < 1 || c->clip_axis > 6) return 0;
  const int oaxis = c->clip_axis, ax = (oaxis - 1) / 2;
  // the corners in (sub-)volume space, clamped to the box (:810-821; the whole volume: fPos = 0), float as there
  float q[4][3];
  for (int k = 0; k < 4; ++k)
    for (int a = 0; a < 3; ++a) {
      const float v = c->clip_slice_corners[k][a];
      q[k][a] = v < 0.0f ? 0.0f : (v > c->fsize[a] ? c->fsize[a] : v);
    }
  const float dv = c->clip_slice_dv;
  int pass = clip_case(oaxis, dv, q[0][ax], c->fsize[ax]) ? 1 : clip_case(oaxis, -dv, q[0][ax], c->fsize[ax]) ? 2 : 0;
  // with shadows the slices may run away from the viewer (axis[3] > 0): no before pass then (:360); the after pass is
  // drawn either way (:400-424)
  if (pass == 1 && c->shadow_on && smk_shadow_light_along_view(c)) pass = 0;
  c->clip_slice_pass = pass;
  if (!pass) return 0;
  const bool blend_max = P.blend == SMK_BLEND_MAX;  // (the blend the ray-marchers used: a frame with shadows follows its light)
  if (pass == 2 && blend_max && c->nranks > 1)
    FAIL(c, "smk_render: the clip slice's after pass under SMK_BLEND_MAX cannot be merged by a maximum (unsharded contexts only)");
  int look = CS_NV20;
  if (c->clip_slice_look == SMK_CLIP_LOOK_R8K) {
    switch (c->dmode) {  // the texture createBricks makes of the data mode (R8kVolRen3D.cpp:1950-2017)
      case SMK_GDM_V1: case SMK_GDM_VGH_V: look = CS_R8K_1B; break;
      case SMK_GDM_V1G: case SMK_GDM_V2: case SMK_GDM_VGH_VG: look = CS_R8K_2B; break;
      case SMK_GDM_V1GH: case SMK_GDM_V2G: case SMK_GDM_V2GH: case SMK_GDM_V3: case SMK_GDM_V3G: case SMK_GDM_V4: case SMK_GDM_VGH:
        look = CS_R8K_4B;
        break;
      default: FAIL(c, "smk_render: the clip slice's R8k look needs a known data mode (the renderer makes no texture of mode %d)", c->dmode);
    }
  }
  const float off = (oaxis - 1) % 2 == 0 ? 0.001f : -0.001f;  // "to avoid z-compete when the slice is on top" (:823)
  for (int k = 0; k < 4; ++k) q[k][ax] = q[k][ax] + off;

  // rays in voxel coordinates: X = E + t D(x, y), t = view depth, (x, y) = pixel centre (compute_raycoef's rays, in double)
  double inv[16];
  smk_inverse_affine(inv, c->mv);
  const double n = c->clip[0], l = c->frustum[0], r = c->frustum[1], b = c->frustum[2], t = c->frustum[3];
  double E[3], Dc[3], Dx[3], Dy[3], v[4][3];
  for (int a = 0; a < 3; ++a) {
    const double sa = (double)c->N[a] / (double)c->fsize[a];
    const double R0 = inv[0 + a], R1 = inv[4 + a], R2 = inv[8 + a];
    E[a] = inv[12 + a] * sa - 0.5;
    Dc[a] = (R0 * l + R1 * b - n * R2) / n * sa;
    Dx[a] = R0 * (r - l) / c->W / n * sa;
    Dy[a] = R1 * (t - b) / c->H / n * sa;
    for (int k = 0; k < 4; ++k) v[k][a] = (double)q[k][a] * sa - 0.5;
  }
  ClipSliceArg Q;
  memset(&Q, 0, sizeof Q);
  for (int a = 0; a < 3; ++a) Q.v0[a] = v[0][a];
  for (int tri = 0; tri < 2; ++tri) {
    double e1[3], e2[3], T[3], A[3], B[3], Nn[3];
    for (int a = 0; a < 3; ++a) {
      e1[a] = v[1 + tri][a] - v[0][a];
      e2[a] = v[2 + tri][a] - v[0][a];
      T[a] = E[a] - v[0][a];
      Q.e1[tri][a] = e1[a];
      Q.e2[tri][a] = e2[a];
    }
    cross3(A, e2, T);
    cross3(B, T, e1);
    cross3(Nn, e2, e1);
    Q.un[tri][0] = dot3(A, Dc); Q.un[tri][1] = dot3(A, Dx); Q.un[tri][2] = dot3(A, Dy);
    Q.wn[tri][0] = dot3(B, Dc); Q.wn[tri][1] = dot3(B, Dx); Q.wn[tri][2] = dot3(B, Dy);
    Q.det[tri][0] = dot3(Nn, Dc); Q.det[tri][1] = dot3(Nn, Dx); Q.det[tri][2] = dot3(Nn, Dy);
    Q.tn[tri] = dot3(e2, B);
    if (Q.tn[tri] == 0) Q.det[tri][0] = Q.det[tri][1] = Q.det[tri][2] = 0;  // (the eye lies in the triangle's plane: never hit)
    if (Q.tn[tri] < 0) {  // (one sign for all four: a hit in front of the eye then has det > 0)
      Q.tn[tri] = -Q.tn[tri];
      for (int k = 0; k < 3; ++k) {
        Q.un[tri][k] = -Q.un[tri][k];
        Q.wn[tri][k] = -Q.wn[tri][k];
        Q.det[tri][k] = -Q.det[tri][k];
      }
    }
  }
  // the screen bounding box of the four projected corners (a pixel of slack); a quad wholly behind the eye or off the
  // window launches nothing, one that crosses the eye's plane takes the whole window
  double bx0 = 1e300, bx1 = -1e300, by0 = 1e300, by1 = -1e300;
  int behind = 0;
  for (int k = 0; k < 4; ++k) {
    const double *M = c->mv, x = q[k][0], y = q[k][1], z = q[k][2];
    const double xe = M[0] * x + M[4] * y + M[8] * z + M[12], ye = M[1] * x + M[5] * y + M[9] * z + M[13];
    const double w = -(M[2] * x + M[6] * y + M[10] * z + M[14]);
    if (!(w > 1e-9 * n)) {
      ++behind;
      continue;
    }
    const double px = (xe * n / w - l) / (r - l) * c->W, py = (ye * n / w - b) / (t - b) * c->H;
    bx0 = std::min(bx0, px); bx1 = std::max(bx1, px);
    by0 = std::min(by0, py); by1 = std::max(by1, py);
  }
  if (behind == 4) return 0;
  if (behind) {
    bx0 = by0 = 0;
    bx1 = c->W;
    by1 = c->H;
  }
  if (!(bx1 >= 0 && by1 >= 0 && bx0 <= c->W && by0 <= c->H)) return 0;
  Q.x0 = (int)std::max(floor(bx0) - 1.0, 0.0) & ~15;
  Q.y0 = (int)std::max(floor(by0) - 1.0, 0.0) & ~15;
  Q.x1 = (int)std::min(ceil(bx1) + 1.0, (double)c->W - 1.0);
  Q.y1 = (int)std::min(ceil(by1) + 1.0, (double)c->H - 1.0);
  if (Q.x1 < Q.x0 || Q.y1 < Q.y0) return 0;
  // Shards (the reference draws the quad per brick, clamped to the brick, :810-821): a rank draws the hit points of its own
  // region -- half-open like the samples', an inner upper face belongs to the neighbour -- and composes them with its own
  // volume frame.  The ordered merge then gives the unsharded frame: along a pixel's ray everything beyond the slice (before
  // pass) or in front of it (after pass) is clipped away in EVERY rank, so the ranks on that side contribute nothing to
  // the pixel, the owner's layer is its volume over the slice (or the slice over its volume), and the ranks on the other
  // side are composited with that layer exactly where the unsharded frame composites their samples.  (That is the
  // geometry's pass: a dv that asks for the other one is obeyed per rank, and the merge is then not the unsharded frame's.)
  // The region is the rank's box WITHOUT the clip plane's cut: the quad stands just outside what the plane keeps.
  for (int a = 0; a < 3; ++a) {
    Q.own_lo[a] = (float)c->g0[a] - 0.5f;
    const float hi = (float)c->g1[a] - 0.5f;
    Q.own_hi[a] = c->g1[a] == c->N[a] ? hi : nextafterf(hi, -INFINITY);
  }
  Q.alpha = c->clip_slice_alpha;
  Q.pass = pass;
  Q.blend_max = blend_max ? 1 : 0;
  const dim3 grid((Q.x1 - Q.x0) / 16 + 1, (Q.y1 - Q.y0) / 16 + 1);
  if (c->dtype == SMK_U8) launch_look<0>(look, grid, s, P, Q, P.out);
  else if (c->dtype == SMK_U16) launch_look<2>(look, grid, s, P, Q, P.out);
  else launch_look<1>(look, grid, s, P, Q, P.out);
  HIPCHK(c, hipGetLastError());
  return 0;
}
