// smk_shadow_plan.hip -- frames with shadows, host side: the half-angle slice set-up (smk_shadowcoef), the boxes and margins
// of a shard, what such a frame refuses, the light exchange between shards, and the shadow stage of a frame (smk_frame.hip):
// the light march with its history, or the frame as a launch per slice.  The kernels are smk_shadow.hip's.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "smk_internal.h"

static double dot3d(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The unit view direction, the unit light direction (ldir = -light.pos), the light's distance d0 and the dot product vdl, the
// sign the reference keeps in axis[3] (R8kVolRen3D.cpp:296-324); false where eye == at or the light sits at the origin
static bool view_and_light(const smk_ctx *c, double vd[3], double ld[3], double *light_dist, double *vdl) {
  for (int k = 0; k < 3; ++k) {
    vd[k] = (double)c->at[k] - c->eye[k];
    ld[k] = -(double)c->light_pos[k];
  }
  const double vl = sqrt(dot3d(vd, vd)), d0 = sqrt(dot3d(ld, ld));
  if (!(vl > 0) || !(d0 > 0)) return false;
  for (int k = 0; k < 3; ++k) {
    vd[k] /= vl;
    ld[k] /= d0;
  }
  *light_dist = d0;
  *vdl = dot3d(vd, ld);
  return true;
}

// vdl > 0: the slices run away from the viewer (smk_shadowcoef's front_to_back), for a stage that needs nothing else of
// the set-up (smk_clip_slice.hip); a degenerate light fails the frame itself, with the reason
bool smk_shadow_light_along_view(const smk_ctx *c) {
  double vd[3], ld[3], d0 = 0, vdl = 0;
  return view_and_light(c, vd, ld, &d0, &vdl) && vdl > 0;
}

// Half-angle slicing set-up (R8kVolRen3D.cpp:296-326; light transform LTWidgetRen.cpp:231-291; light-buffer
// coordinates R8kVolRen3D.cpp:1664-1676), everything in double, rounded once: slice planes sn . X = tmin + k dc
// in model space, eye rays X = e + tau (R0 px + R1 py - n R2), light rays from the apex of the light's
// projection, and the model -> light-buffer map.  The CPU checker (orc_shadow_setup) does the same steps.
static int compute_shadowcoef(smk_ctx *c, smk_shadowcoef *o) {
  memset(o, 0, sizeof *o);
  const double f[3] = {c->fsize[0], c->fsize[1], c->fsize[2]}, N[3] = {(double)c->N[0], (double)c->N[1], (double)c->N[2]};
  double vd[3], ld[3], d0 = 0, vdl = 0;
  if (!view_and_light(c, vd, ld, &d0, &vdl)) FAIL(c, "smk_render: shadows need eye != at and a light away from the origin");
  if (vdl <= 0)
    for (int k = 0; k < 3; ++k) vd[k] = -vd[k];
  double h[3];
  for (int k = 0; k < 3; ++k) h[k] = (vd[k] - ld[k]) * .5 + ld[k];
  o->front_to_back = vdl > 0;
  double xf[16], xinv[16];
  for (int i = 0; i < 16; ++i) xf[i] = c->xform[i];
  smk_inverse_affine(xinv, xf);
  double sn[3];
  for (int a = 0; a < 3; ++a) sn[a] = xinv[0 + a] * h[0] + xinv[4 + a] * h[1] + xinv[8 + a] * h[2];
  const double snl = sqrt(dot3d(sn, sn));
  if (!(snl > 0)) FAIL(c, "smk_render: shadows: degenerate half-way vector");
  for (int a = 0; a < 3; ++a) sn[a] /= snl;
  double tmin = 1e300, tmax = -1e300;
  for (int i = 0; i < 8; ++i) {
    const double X[3] = {(i & 1) ? f[0] : 0, (i & 2) ? f[1] : 0, (i & 4) ? f[2] : 0};
    const double t = dot3d(sn, X);
    if (t < tmin) tmin = t;
    if (t > tmax) tmax = t;
  }
  double dc;
  int S;
  if (c->steps > 0) {
    S = c->steps;
    dc = (tmax - tmin) / S;
  } else {
    const float disf = c->fsize[0] / ((float)c->N[0] * c->sample_rate);  // R8kVolRen3D.cpp:1330
    dc = disf;
    S = (int)((tmax - tmin) / dc);
  }
  if (S < 0) S = 0;
  o->nslices = S;
  double inv[16];
  smk_inverse_affine(inv, c->mv);
  const double n = c->clip[0];
  const double l = c->frustum[0], r = c->frustum[1], b = c->frustum[2], t = c->frustum[3];
  o->pxs = (float)((r - l) / c->W);
  o->pxl = (float)l;
  o->pys = (float)((t - b) / c->H);
  o->pyl = (float)b;
  const double R0[3] = {inv[0], inv[1], inv[2]}, R1[3] = {inv[4], inv[5], inv[6]}, R2[3] = {inv[8], inv[9], inv[10]};
  const double e[3] = {inv[12], inv[13], inv[14]};
  for (int a = 0; a < 3; ++a) {
    const double s = N[a] / f[a];
    o->Ec[a] = (float)(e[a] * s - 0.5);
    o->Dx[a] = (float)(R0[a] * s);
    o->Dy[a] = (float)(R1[a] * s);
    o->Dc[a] = (float)(-n * R2[a] * s);
  }
  o->nDx = (float)dot3d(sn, R0);
  o->nDy = (float)dot3d(sn, R1);
  o->nDc = (float)(-n * dot3d(sn, R2));
  o->num0 = (float)(tmin - dot3d(sn, e));
  o->dnum = (float)dc;
  // light view: x' = s.q, y' = u.q, z' = 1 - F.q, w = 1 + z'/d0 for a world point q = xform (X - f/2)
  const double F[3] = {-ld[0], -ld[1], -ld[2]};
  double sv[3] = {F[1] * 0 - F[2] * 1, F[2] * 0 - F[0] * 0, F[0] * 1 - F[1] * 0};
  const double sl = sqrt(dot3d(sv, sv));
  if (!(sl > 1e-12)) FAIL(c, "smk_render: shadows: a light on the y axis has no light transform (gluLookAt with up = y, LTWidgetRen.cpp:262-276)");
  for (int k = 0; k < 3; ++k) sv[k] /= sl;
  const double uv[3] = {sv[1] * F[2] - sv[2] * F[1], sv[2] * F[0] - sv[0] * F[2], sv[0] * F[1] - sv[1] * F[0]};
  double rowx[4], rowy[4], roww[4];
  for (int a = 0; a < 3; ++a) {
    const double col[3] = {xf[4 * a + 0], xf[4 * a + 1], xf[4 * a + 2]};
    rowx[a] = dot3d(sv, col);
    rowy[a] = dot3d(uv, col);
    roww[a] = -dot3d(F, col) / d0;
  }
  {
    const double tcol[3] = {xf[12], xf[13], xf[14]};
    rowx[3] = dot3d(sv, tcol);
    rowy[3] = dot3d(uv, tcol);
    roww[3] = 1.0 + (1.0 - dot3d(F, tcol)) / d0;
    for (int a = 0; a < 3; ++a) {
      rowx[3] -= rowx[a] * f[a] * .5;
      rowy[3] -= rowy[a] * f[a] * .5;
      roww[3] -= roww[a] * f[a] * .5;
    }
  }
  double cx = rowx[3], cy = rowy[3], cw = roww[3];
  for (int a = 0; a < 3; ++a) {
    const double sc = f[a] / N[a];
    o->Xm[a] = (float)(rowx[a] * sc);
    o->Ym[a] = (float)(rowy[a] * sc);
    o->Wm[a] = (float)(roww[a] * sc);
    cx += rowx[a] * sc * .5;
    cy += rowy[a] * sc * .5;
    cw += roww[a] * sc * .5;
  }
  o->Xm[3] = (float)cx;
  o->Ym[3] = (float)cy;
  o->Wm[3] = (float)cw;
  const double LBf = (double)c->shadow_q * (double)c->shadow_px;
  o->LB = (int)ceil(LBf);
  if (o->LB < 1) FAIL(c, "smk_render: shadows: empty light buffer");
  o->lscale = (float)(.85 * LBf);
  o->lbias = (float)(.5 * LBf);
  o->las = (float)(1.0 / (.85 * LBf));
  o->lal = (float)(-.5 / .85);
  double apex[3], gx[3], gy[3], gc[3];
  for (int a = 0; a < 3; ++a) {
    apex[a] = xinv[12 + a] + f[a] * .5;
    gx[a] = gy[a] = gc[a] = 0;
    for (int k = 0; k < 3; ++k) {
      apex[a] += xinv[4 * k + a] * F[k] * (1.0 + d0);
      gx[a] += xinv[4 * k + a] * sv[k];
      gy[a] += xinv[4 * k + a] * uv[k];
      gc[a] += xinv[4 * k + a] * F[k] * -d0;
    }
  }
  for (int a = 0; a < 3; ++a) {
    const double s = N[a] / f[a];
    o->Lc[a] = (float)(apex[a] * s - 0.5);
    o->Gx[a] = (float)(gx[a] * s);
    o->Gy[a] = (float)(gy[a] * s);
    o->Gc[a] = (float)(gc[a] * s);
  }
  o->nGx = (float)dot3d(sn, gx);
  o->nGy = (float)dot3d(sn, gy);
  o->nGc = (float)dot3d(sn, gc);
  o->lnum0 = (float)(tmin - dot3d(sn, apex));
  o->ldnum = (float)dc;
  return 0;
}

extern "C" int smk_set_shadow(smk_ctx *c, int on, int buffer_px, float quality) {
  if (!c) return 1;
  if (on && (buffer_px < 1 || buffer_px > 8192 || !(quality > 0.0f) || quality > 1.0f))
    FAIL(c, "smk_set_shadow: buffer_px in 1..8192 and quality in (0,1] (gluvvui.cpp:156-167 clamps the qualities to [.1,1])");
  c->shadow_on = on ? 1 : 0;
  if (on) {
    c->shadow_px = buffer_px;
    c->shadow_q = quality;
  }
  return 0;
}

extern "C" int smk_get_shadowcoef(smk_ctx *c, smk_shadowcoef *out) {
  if (!c || !out) return 1;
  if (!c->have_volume || !c->have_camera) FAIL(c, "smk_get_shadowcoef: volume and camera must be set");
  return compute_shadowcoef(c, out);
}

extern "C" int smk_get_light_buffer(smk_ctx *c, float *rgba_out, int *lb_out) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->light_lb || !c->d_light_last) FAIL(c, "smk_get_light_buffer: no frame with shadows has been rendered");
  if (lb_out) *lb_out = c->light_lb;
  if (rgba_out) {
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(rgba_out, c->d_light_last, (size_t)c->light_lb * c->light_lb * 16, hipMemcpyDeviceToHost));
  }
  return 0;
}

// The light's BSP order: from the apex of the light rays (smk_shadowcoef Lc, voxel index space), the point every light-buffer
// texel's ray starts from -- a ray crosses the shards' convex boxes in this order (R8kVolRen3D.cpp:582-679 draws the bricks of
// a shadowed volume one after another against one light buffer)
extern "C" int smk_shard_light_order(smk_ctx *c, int *order) {
  if (!c || !order) return 1;
  if (!c->have_volume || !c->have_camera) FAIL(c, "smk_shard_light_order: volume and camera must be set");
  smk_shadowcoef sc;
  if (compute_shadowcoef(c, &sc)) return 1;
  const double l[3] = {sc.Lc[0], sc.Lc[1], sc.Lc[2]};
  smk_bsp_order(c, l, order);
  return 0;
}

// Margin m of a shard with shadows ("Shadows on shards"): an eye sample p of slice k looks the light buffer up
// bilinearly at p's light-buffer position, i.e. the (up to) 4 texels whose centres lie less than one texel from it on each
// axis; each such texel's slice-k sample lies on slice k's plane near p, off by the texel offset times the Jacobian of the
// map (buffer position -> point of the plane), here (a, b) -> Lc + lnum G(a, b) / nG(a, b).  Its largest size over a grid
// of the region's box, in voxels per texel, with half again as much for the curvature between grid points and the float
// chains, rounded up: the light samples rank j must march itself lie within m voxels of its region.
static int shadow_margin(const smk_shadowcoef &sc, const int g0[3], const int g1[3]) {
  double worst = 0.0;
  const int n = 8;
  for (int iz = 0; iz <= n; ++iz)
    for (int iy = 0; iy <= n; ++iy)
      for (int ix = 0; ix <= n; ++ix) {
        const int ii[3] = {ix, iy, iz};
        double p[3];
        for (int a = 0; a < 3; ++a) p[a] = (double)g0[a] - 0.5 + (double)(g1[a] - g0[a]) * ii[a] / n;
        const double lw = sc.Wm[0] * p[0] + sc.Wm[1] * p[1] + sc.Wm[2] * p[2] + sc.Wm[3];
        if (!(fabs(lw) > 1e-30)) return 1 << 20;
        const double lx = (sc.Xm[0] * p[0] + sc.Xm[1] * p[1] + sc.Xm[2] * p[2] + sc.Xm[3]) / lw * sc.lscale + sc.lbias;
        const double ly = (sc.Ym[0] * p[0] + sc.Ym[1] * p[1] + sc.Ym[2] * p[2] + sc.Ym[3]) / lw * sc.lscale + sc.lbias;
        const double a = lx * sc.las + sc.lal, b = ly * sc.las + sc.lal;  // (texel x has a = fma(x + .5, las, lal))
        double G[3], d[3], gg = 0.0, dg = 0.0;
        for (int q = 0; q < 3; ++q) {
          G[q] = a * sc.Gx[q] + b * sc.Gy[q] + sc.Gc[q];
          d[q] = p[q] - sc.Lc[q];
          gg += G[q] * G[q];
          dg += d[q] * G[q];
        }
        const double nG = a * sc.nGx + b * sc.nGy + sc.nGc;
        if (!(gg > 0.0) || !(fabs(nG) > 1e-30)) return 1 << 20;
        const double w = dg / gg;  // p = Lc + w G
        for (int q = 0; q < 3; ++q) {
          const double ja = w * (sc.Gx[q] - G[q] * sc.nGx / nG), jb = w * (sc.Gy[q] - G[q] * sc.nGy / nG);
          worst = std::max(worst, (double)sc.las * (fabs(ja) + fabs(jb)));
        }
      }
  const double m = ceil(1.5 * worst + 0.5);
  return m > (double)(1 << 20) || m != m ? 1 << 20 : std::max(1, (int)m);
}

// A frame with shadows: the half-angle slices (compute_shadowcoef), the eye rays over them in P.sh, and the boxes.  On the
// whole volume: a light sample lies in the volume's closed box (what an orthogonal clip plane leaves of it), an eye sample in
// that box widened by SMK_SHADOW_BOX_EPS.  On a shard the outer faces keep that treatment and the inner ones the half-open
// rule of a shard's region (a sample on the split plane belongs to the upper half), so that every light sample and every eye
// sample of the unsharded frame belongs to exactly one rank; the light march's bracket and sample set stay the whole volume's
// (P.sh.llo / lhi).  With S: the phase-1 / phase-2 parameters of the shard (SmkShadowShard), *halo_need = m + 1.
int smk_shadow_setup(smk_ctx *c, RenderParams &P, smk_shadowcoef &sc, SmkShadowShard *S, int *halo_need) {
  if (compute_shadowcoef(c, &sc)) return 1;
  // the eye rays over the half-angle slices, planes counted from the eye (smk_internal.h SmkShadowRays)
  SmkShadowRays &h = P.sh;
  memset(&h, 0, sizeof h);
  // (option shadow_look 1, the NV20 look: on = 2, and keep = 1 - amb, the share of its colour a fully shadowed sample loses)
  h.on = c->opt_shadow_look ? 2 : 1;
  h.keep = c->opt_shadow_look ? 1.0f - c->amb : 0.0f;
  for (int a = 0; a < 3; ++a) { h.Ec[a] = sc.Ec[a]; h.Dc[a] = sc.Dc[a]; h.Dx[a] = sc.Dx[a]; h.Dy[a] = sc.Dy[a]; }
  h.nDc = sc.nDc; h.nDx = sc.nDx; h.nDy = sc.nDy;
  if (sc.front_to_back) { h.numA = fmaf(1.0f, sc.dnum, sc.num0); h.dB = sc.dnum; h.k0 = 1; h.dk = 1; }
  else { h.numA = fmaf((float)sc.nslices, sc.dnum, sc.num0); h.dB = -sc.dnum; h.k0 = sc.nslices; h.dk = -1; }
  h.LB = sc.LB;
  for (int q = 0; q < 4; ++q) { h.Xm[q] = sc.Xm[q]; h.Ym[q] = sc.Ym[q]; h.Wm[q] = sc.Wm[q]; }
  h.lscale = sc.lscale; h.lbias = sc.lbias;
  {
    smk_raycoef &rc = P.rc;
    memset(&rc, 0, sizeof rc);
    rc.pxs = sc.pxs; rc.pxl = sc.pxl; rc.pys = sc.pys; rc.pyl = sc.pyl;
    rc.nplanes = sc.nslices;
    // (Bc: the central ray's step, which the kernel choice below keys its measurements on)
    const double nDc = (double)sc.nDc != 0.0 ? (double)sc.nDc : 1.0;
    for (int a = 0; a < 3; ++a) rc.Bc[a] = (float)((double)h.dB / nDc * (double)sc.Dc[a]);
  }
  // The last slice lies ON the volume's far corner -- on a whole face when the half-way vector is a volume axis (a light at
  // the eye) -- where a sample's coordinate, the end of an fma chain, lands on either side of the face by rounding.  The
  // reference draws that slice (a polygon clipped against the box keeps its boundary); the eye pass's membership test is
  // therefore 2^-10 voxels wide of the box (clamp-to-edge fetches: the value at the face).  The CPU checker does the same.
  // The light pass draws the same polygon, so a light ray's sample is tested against the same widened box: with a closed
  // box the light samples of a face-coincident last slice fell outside by rounding and the slice was missing from the
  // light buffer alone (tests/test_shadow_witness.py::test_face_coincident_last_slice).  Clip planes: both passes draw
  // the same clipped slice polygons in the reference (volShadow slices the box setupClips left; glClipPlane stays
  // enabled), so a light ray's sample must lie in the same box and on the kept side of the free plane.
  // A sub-box (smk_set_region) is to both passes what an orthogonal clip plane's box is: smk_region_box has intersected it into
  // the eye box (P.lo / P.hi) and, below, into the light box; its faces are outer ones, closed and widened like a clip face --
  // the half-open upper face of an unshadowed sub-box frame is a shard's rule, and a sub-box never meets a shard here
  // (shadow_refusals).  The slice set stays the whole volume's (compute_shadowcoef).
  if (c->region_on && c->nranks == 1)
    for (int a = 0; a < 3; ++a) P.top[a] = 1;
  float wlo[3], whi[3];
  int wtop[3];
  const int z0[3] = {0, 0, 0};
  smk_region_box(c, z0, c->N, wlo, whi, wtop);
  float olo[3], ohi[3];
  for (int a = 0; a < 3; ++a) {
    const bool inner_lo = c->g0[a] > 0 && P.lo[a] == (float)c->g0[a] - 0.5f, inner_hi = !P.top[a];
    h.llo[a] = wlo[a] - SMK_SHADOW_BOX_EPS;
    h.lhi[a] = whi[a] + SMK_SHADOW_BOX_EPS;
    olo[a] = inner_lo ? P.lo[a] : P.lo[a] - SMK_SHADOW_BOX_EPS;
    ohi[a] = inner_hi ? nextafterf(P.hi[a], -INFINITY) : P.hi[a] + SMK_SHADOW_BOX_EPS;
    if (!inner_lo) P.lo[a] -= SMK_SHADOW_BOX_EPS;
    if (inner_hi) P.hin[a] = nextafterf(P.hi[a], -INFINITY);
    else {
      P.hi[a] += SMK_SHADOW_BOX_EPS;
      P.hin[a] = P.hi[a];
      P.top[a] = 1;
    }
  }
  if (!S) return 0;
  memset(S, 0, sizeof *S);
  S->nranks = c->nranks;
  S->rank = c->rank;
  for (int a = 0; a < 3; ++a) { S->olo[a] = olo[a]; S->ohi[a] = ohi[a]; }
  int m_own = 0;
  for (int j = 0; j < c->nranks; ++j) {
    int g0[3], g1[3];
    smk_shard_region(c, j, g0, g1);
    const int m = shadow_margin(sc, g0, g1);
    if (j == c->rank) m_own = m;
    for (int a = 0; a < 3; ++a) {
      S->glo[j][a] = (float)((double)g0[a] - 0.5 - m);
      S->ghi[j][a] = (float)((double)g1[a] - 0.5 + m);
    }
  }
  for (int a = 0; a < 3; ++a) {
    S->xlo[a] = S->glo[c->rank][a] - 0.25f;
    S->xhi[a] = S->ghi[c->rank][a] + 0.25f;
  }
  const double l[3] = {sc.Lc[0], sc.Lc[1], sc.Lc[2]};
  smk_bsp_order(c, l, S->order);
  if (halo_need) *halo_need = m_own + 1;
  return 0;
}

// what a frame with shadows cannot be combined with (the same reasons as smk_render's)
static int shadow_refusals(smk_ctx *c, const RenderParams &P) {
  const int sk = smk_shade_kind(c);
  const bool nv20 = c->opt_shadow_look != 0;  // (option shadow_look 1: NV20VolRen3D2's look, smk.h smk_set_shadow)
  if (c->tf_mode == 0 && nv20) FAIL(c, "smk_render: shadow_look 1 needs a 2-D or 3-D transfer function (the 1-D table renderer has no shadow mode)");
  if (c->tf_mode == 0) FAIL(c, "smk_render: shadows need a 2-D or 3-D transfer function (the 1-D table renderer has no shadow mode)");
  if (sk == 2 && !nv20) FAIL(c, "smk_render: shadows are implemented for R8k shading or none (NV20 combiners: no shadow mode in NV20VolRen3D)");
  if (sk == 1 && nv20) FAIL(c, "smk_render: shadow_look 1 is NV20VolRen3D2's: shading none or NV20");
  if (nv20 && !(c->amb >= 0.0f && c->amb <= 1.0f))
    FAIL(c, "smk_render: shadow_look 1 needs the ambient term of smk_set_shading finite and in [0, 1] (amb = %g)", (double)c->amb);
  if (nv20 && P.pert_on) FAIL(c, "smk_render: shadow_look 1 has no perturbed instances (perturbation under shadows is the R8k look's, option shadow_perturb)");
  if (nv20 && (c->opt_lockstep & 256)) FAIL(c, "smk_render: shadow_look 1 has no shadow_fused instances; use the two marches or shadow_march 0");
  if (nv20 && c->opt_kernel == 3) FAIL(c, "smk_render: shadow_look 1: the column-stream kernel has no shadow mode");
  if (c->nranks > 1 && (!c->opt_shadow_march || (c->opt_lockstep & 256)))
    FAIL(c, "smk_render: shadows need the whole volume on one GPU with option shadow_march 0 or shadow_fused (the light buffer couples every "
            "slice of every brick); a shard renders shadows with the two marches only");
  // (perturbed fetches under shadows are opt-in, option shadow_perturb: smk.h smk_set_shadow says why)
  if (P.pert_on && !c->opt_shadow_perturb) FAIL(c, "smk_render: shadows cannot be combined with perturbation or a sub-box");
  if (c->nranks > 1 && (P.pert_on || c->region_on))
    FAIL(c, "smk_render: shadows on shards cannot be combined with perturbation or a sub-box (the light exports and the grown boxes "
            "of a shard know neither); render the whole volume on one GPU");
  if ((c->opt_lockstep & 256) && (P.pert_on || c->region_on))
    FAIL(c, "smk_render: option shadow_fused has no perturbed instances and no sub-box; use the two marches or shadow_march 0");
  if (c->opt_kernel == 3) FAIL(c, "smk_render: the column-stream kernel has no shadow mode");
  if (c->dtype == SMK_U16 && (!c->opt_shadow_march || (c->opt_lockstep & 256)))
    FAIL(c, "smk_render: u16 voxels render shadows with the two marches only (no shadow_march 0 or shadow_fused instances)");
  return 0;
}

// a shard's halo against the margin of its frame with shadows
static int shadow_halo_check(smk_ctx *c, int need) {
  const int have = smk_step_shown_halo(c);  // (of the SHOWN step: a sharded stencil producer leaves fewer exact halo voxels than it found)
  for (int a = 0; a < 3; ++a)
    if (have < need && c->D[a] < c->N[a]) {
      if (have != c->halo)
        FAIL(c, "smk_render: shadows on a shard need halo >= %d voxels (time step %d has a valid halo of %d, of option halo %d: "
                "smk_get_timestep_halo; margin %d, smk_get_shadow_margin); set option 'halo' before upload", need, c->ts_cur_id, have, c->halo, need - 1);
      FAIL(c, "smk_render: shadows on a shard need halo >= %d voxels (have %d; margin %d, smk_get_shadow_margin); set option 'halo' before upload",
           need, c->halo, need - 1);
    }
  return 0;
}

// The light march keeps every slice's light buffer: (nslices + 1) buffers of hstride texels, nhist in all.  Where that does not
// fit (more than a quarter of the device's free memory, or 32 GB) the frame is a launch per slice, as with the option off.
static bool light_history_fits(smk_ctx *c, size_t nhist) {
  if (nhist <= c->light_hist_cap) return true;
  size_t fr = 0, tot = 0;
  if (c->d_light_hist) (void)hipFree(c->d_light_hist);
  c->d_light_hist = nullptr;
  c->light_hist_cap = 0;
  c->d_light_last = nullptr;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess || nhist * 16 > fr / 4 || nhist * 16 > ((size_t)32 << 30) ||
      hipMalloc((void **)&c->d_light_hist, nhist * 16) != hipSuccess) {
    (void)hipGetLastError();
    c->d_light_hist = nullptr;
    return false;
  }
  c->light_hist_cap = nhist;
  return true;
}

// the light march into the history (the whole volume's, or a shard's from its light entries S); ev0 opens the frame's
// kernel-time bracket before it, and the eye pass is then an ordinary frame of the ray-marchers over P.sh
static int light_march(smk_ctx *c, RenderParams &P, const smk_shadowcoef &sc, const SmkShadowShard &S, size_t hstride, hipStream_t s) {
  HIPCHK(c, hipEventRecord(c->ev0, s));
  hipError_t e = c->nranks > 1 ? smk_launch_shadow_march_shard(P, sc, c->dtype, c->tf_mode, c->d_light_hist, (long long)hstride, S, s)
                               : smk_launch_shadow_march(P, sc, c->dtype, c->tf_mode, c->d_light_hist, (long long)hstride, s);
  if (e == hipErrorNotSupported) FAIL(c, "smk_render: no shadow kernel instance for this configuration");
  HIPCHK(c, e);
  P.sh.hist = c->d_light_hist;
  P.sh.hstride = (long long)hstride;
  c->light_hist_n = sc.nslices + 1;
  c->light_hist_stride = (long long)hstride;
  c->d_light_last = c->d_light_hist + (size_t)sc.nslices * hstride;
  // the history is written once (16 B per texel and slice)
  c->last_alg_bytes += (double)sc.nslices * (16.0 * (double)((size_t)sc.LB * sc.LB));
  return 0;
}

// the whole frame as a launch per slice (option shadow_march 0, shadow_fused, or a history that does not fit), between two
// light buffers used in turn
static int launch_per_slice(smk_ctx *c, const RenderParams &P, const smk_shadowcoef &sc, void *d_rgba, void *d_depth, hipStream_t s) {
  const size_t nl = (size_t)sc.LB * sc.LB;
  if (nl > c->light_cap) {
    for (int k = 0; k < 2; ++k) {
      if (c->d_light[k]) (void)hipFree(c->d_light[k]);
      c->d_light[k] = nullptr;
      HIPCHK(c, hipMalloc((void **)&c->d_light[k], nl * 16));
    }
    c->light_cap = nl;
    c->d_light_last = nullptr;
  }
  HIPCHK(c, hipEventRecord(c->ev0, s));
  HIPCHK(c, hipMemsetAsync(c->d_light[0], 0, nl * 16, s));
  HIPCHK(c, hipMemsetAsync(d_rgba, 0, (size_t)c->W * c->H * 16, s));
  if (d_depth) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)d_depth, 0x7f800000, (size_t)c->W * c->H, s));  // (+inf: no sample yet)
  if (!c->d_shadow_barrier) HIPCHK(c, hipMalloc((void **)&c->d_shadow_barrier, 16 * 9 * 4));  // (the common word + one per XCD, a cache line apart)
  hipError_t e = smk_launch_shadow(P, sc, c->dtype, c->tf_mode, smk_shade_kind(c), c->d_light[0], c->d_light[1], c->d_shadow_barrier, s);
  if (e == hipErrorNotSupported) FAIL(c, "smk_render: no shadow kernel instance for this configuration");
  HIPCHK(c, e);
  c->d_light_last = c->d_light[sc.nslices & 1];
  // per slice the frame buffer (read + write where the slice covers it) and both light buffers move again
  c->last_alg_bytes += (double)sc.nslices * (32.0 * (double)nl);
  c->last_kernel = 3;
  return 0;
}

// The shadow stage of a frame (half-angle slicing, smk_shadow.hip): the light march, then the eye pass as an ordinary frame of
// the ray-marchers over the half-angle slices (SmkShadowRays in P.sh; *marched) -- or, option shadow_march 0, the whole frame
// as a launch per slice.  A shard's frame needs this frame's light entries and a halo as wide as its margin.
int smk_shadow_frame(smk_ctx *c, RenderParams &P, void *d_rgba, void *d_depth, hipStream_t s, bool *marched) {
  const int sk = smk_shade_kind(c);
  // (a perturbed or sub-box frame on a shard is refused for what it is, entries or none: shadow_refusals)
  if (c->nranks > 1 && !c->shadow_entries_fresh && c->tf_mode != 0 && sk != (c->opt_shadow_look ? 1 : 2) && !((P.pert_on && c->opt_shadow_perturb) || c->region_on))
    FAIL(c, "smk_render: shadows need the whole volume on one GPU (the light buffer couples every slice of every brick) -- "
            "or, on a shard, this frame's light entries: smk_shadow_exports_device on every rank, then smk_shadow_entries_device "
            "(smk_shadow_exchange_local in one process)");
  const bool entries = c->shadow_entries_fresh;
  c->shadow_entries_fresh = false;  // (consumed by this frame, whatever becomes of it)
  if (shadow_refusals(c, P)) return 1;
  smk_shadowcoef sc;
  SmkShadowShard S;
  int halo_need = 0;
  if (smk_shadow_setup(c, P, sc, c->nranks > 1 ? &S : nullptr, &halo_need)) return 1;
  if (c->nranks > 1) {
    if (shadow_halo_check(c, halo_need)) return 1;
    if (!entries || memcmp(&sc, &c->shadow_entries_sc, sizeof sc))
      FAIL(c, "smk_render: shadows on a shard: the light entries were made for another slice set (camera, light or buffer changed since)");
    S.entries = c->d_shadow_entries;
  }
  P.blend = SMK_BLEND_FRONT_TO_BACK;  // (a light that faces the viewer: the per-slice form blends back to front, the marchers
                                      //  composite the same samples front to back -- the association of the blend differs)
  // (buffers 4 KiB + 256 B further apart than their size: 512^2 texels are exactly 4 MiB, and a wave of the light march
  //  stores to 8 consecutive buffers at once -- a power-of-two stride could put them all into the same memory channels;
  //  measured: 1.00 ms with the pad, 1.03 without, i.e. the fabric's address hash already spreads them)
  const size_t hstride = (size_t)sc.LB * sc.LB + 272;
  const size_t nhist = hstride * ((size_t)sc.nslices + 1);
  *marched = c->opt_shadow_march && !(c->opt_lockstep & 256) && sc.nslices > 0 && light_history_fits(c, nhist);
  c->light_lb = sc.LB;
  c->light_hist_n = 0;
  if (c->nranks > 1 && !*marched)
    FAIL(c, "smk_render: shadows on a shard: the light history (%.1f GB) does not fit a quarter of the free device memory",
         (double)nhist * 16.0 / 1e9);
  return *marched ? light_march(c, P, sc, S, hstride, s) : launch_per_slice(c, P, sc, d_rgba, d_depth, s);
}

float4 *smk_shadow_entries_reserve(smk_ctx *c, int LB) {
  const size_t n = (size_t)c->nranks * LB * LB;
  if (n > c->shadow_entries_cap) {
    if (c->d_shadow_entries) (void)hipFree(c->d_shadow_entries);
    c->d_shadow_entries = nullptr;
    c->shadow_entries_cap = 0;
    if (hipMalloc((void **)&c->d_shadow_entries, n * 16) != hipSuccess) {
      (void)hipGetLastError();
      c->d_shadow_entries = nullptr;
      return nullptr;
    }
    c->shadow_entries_cap = n;
  }
  c->shadow_entries_fresh = false;
  return c->d_shadow_entries;
}

void smk_shadow_entries_commit(smk_ctx *c, const smk_shadowcoef &sc) {
  c->shadow_entries_sc = sc;
  c->shadow_entries_fresh = true;
}

int smk_shadow_shard_setup(smk_ctx *c, RenderParams &P, smk_shadowcoef &sc, SmkShadowShard &S, hipStream_t s) {
  if (!c->shadow_on) FAIL(c, "smk_shadow_exports_device: shadows are off (smk_set_shadow)");
  if (smk_build_params(c, P, s)) return 1;
  if (shadow_refusals(c, P)) return 1;
  int need = 0;
  if (smk_shadow_setup(c, P, sc, &S, &need)) return 1;
  if (shadow_halo_check(c, need)) return 1;
  return 0;
}

extern "C" int smk_shadow_exports_device(smk_ctx *c, void *d_exports, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!d_exports) FAIL(c, "smk_shadow_exports_device: null output");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  RenderParams P;
  smk_shadowcoef sc;
  SmkShadowShard S;
  if (smk_shadow_shard_setup(c, P, sc, S, s)) return 1;
  S.exports = (float4 *)d_exports;
  hipError_t e = smk_launch_shadow_exports(P, sc, c->dtype, c->tf_mode, S, s);
  if (e == hipErrorNotSupported) FAIL(c, "smk_shadow_exports_device: no shadow kernel instance for this configuration");
  HIPCHK(c, e);
  return smk_step_mark_used(c, s);
}

extern "C" int smk_shadow_entries_device(smk_ctx *c, const void *d_entries, void *stream) {
  if (!c) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!d_entries) FAIL(c, "smk_shadow_entries_device: null input");
  if (!c->have_volume || !c->have_camera) FAIL(c, "smk_shadow_entries_device: volume and camera must be set");
  hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  smk_shadowcoef sc;
  if (compute_shadowcoef(c, &sc)) return 1;
  float4 *d = smk_shadow_entries_reserve(c, sc.LB);
  if (!d) FAIL(c, "smk_shadow_entries_device: device allocation failed");
  HIPCHK(c, hipMemcpyAsync(d, d_entries, (size_t)c->nranks * sc.LB * sc.LB * 16, hipMemcpyDeviceToDevice, s));
  smk_shadow_entries_commit(c, sc);
  return 0;
}

extern "C" int smk_get_shadow_margin(smk_ctx *c, int *m, int *halo_needed) {
  if (!c) return 1;
  if (!c->have_volume || !c->have_camera) FAIL(c, "smk_get_shadow_margin: volume and camera must be set");
  smk_shadowcoef sc;
  if (compute_shadowcoef(c, &sc)) return 1;
  const int mm = shadow_margin(sc, c->g0, c->g1);
  if (m) *m = mm;
  if (halo_needed) *halo_needed = mm + 1;
  return 0;
}

int smk_shadow_light_owned(smk_ctx *c, RenderParams &P, smk_shadowcoef &sc, float olo[3], float ohi[3]) {
  if (!c->shadow_on) FAIL(c, "smk_get_stat: light_samples needs shadows on (smk_set_shadow)");
  if (smk_build_params(c, P, c->stream)) return 1;
  SmkShadowShard S;
  if (smk_shadow_setup(c, P, sc, &S, nullptr)) return 1;
  for (int a = 0; a < 3; ++a) { olo[a] = S.olo[a]; ohi[a] = S.ohi[a]; }
  return 0;
}

// In-process transport of the light exchange: phase 1 on every rank into its own scratch buffer, then slot j of rank r's
// exports into slot r of rank j's entries (device-to-device; peer copies between devices).  Synchronous: every rank's stream
// is idle before (the entries of the previous frame are no longer read) and after.
extern "C" int smk_shadow_exchange_local(smk_ctx *const *all, int nranks) {
  if (!all || nranks < 1 || nranks > SMK_MAX_RANKS) return 1;
  for (int r = 0; r < nranks; ++r) {
    if (!all[r]) return 1;
    if (all[r]->nranks != nranks || all[r]->rank != r) FAIL(all[r], "smk_shadow_exchange_local: context %d is not shard %d of %d", r, r, nranks);
  }
  std::vector<smk_shadowcoef> scs(nranks);
  for (int r = 0; r < nranks; ++r) {
    smk_ctx *c = all[r];
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    RenderParams P;
    SmkShadowShard S;
    if (smk_shadow_shard_setup(c, P, scs[r], S, c->stream)) return 1;
    if (r > 0 && memcmp(&scs[r], &scs[0], sizeof scs[0])) FAIL(c, "smk_shadow_exchange_local: the ranks' slice sets differ (camera, light, buffer or volume)");
    const size_t n = (size_t)nranks * scs[r].LB * scs[r].LB;
    if (n > c->shadow_exports_cap) {
      if (c->d_shadow_exports) (void)hipFree(c->d_shadow_exports);
      c->d_shadow_exports = nullptr;
      c->shadow_exports_cap = 0;
      HIPCHK(c, hipMalloc((void **)&c->d_shadow_exports, n * 16));
      c->shadow_exports_cap = n;
    }
    S.exports = c->d_shadow_exports;
    hipError_t e = smk_launch_shadow_exports(P, scs[r], c->dtype, c->tf_mode, S, c->stream);
    if (e == hipErrorNotSupported) FAIL(c, "smk_shadow_exchange_local: no shadow kernel instance for this configuration");
    HIPCHK(c, e);
  }
  const size_t nl = (size_t)scs[0].LB * scs[0].LB;
  std::vector<float4 *> dst(nranks);
  for (int j = 0; j < nranks; ++j) {
    HIPCHK(all[j], hipSetDevice(all[j]->device));
    dst[j] = smk_shadow_entries_reserve(all[j], scs[0].LB);
    if (!dst[j]) FAIL(all[j], "smk_shadow_exchange_local: device allocation failed");
  }
  for (int r = 0; r < nranks; ++r) {
    smk_ctx *c = all[r];
    HIPCHK(c, hipSetDevice(c->device));
    for (int j = 0; j < nranks; ++j) {
      if (all[j]->device == c->device)
        HIPCHK(c, hipMemcpyAsync(dst[j] + (size_t)r * nl, c->d_shadow_exports + (size_t)j * nl, nl * 16, hipMemcpyDeviceToDevice, c->stream));
      else
        HIPCHK(c, hipMemcpyPeerAsync(dst[j] + (size_t)r * nl, all[j]->device, c->d_shadow_exports + (size_t)j * nl, c->device, nl * 16, c->stream));
    }
  }
  for (int r = 0; r < nranks; ++r) {
    HIPCHK(all[r], hipSetDevice(all[r]->device));
    HIPCHK(all[r], hipStreamSynchronize(all[r]->stream));
  }
  for (int j = 0; j < nranks; ++j) smk_shadow_entries_commit(all[j], scs[0]);
  return 0;
}

extern "C" int smk_get_light_history(smk_ctx *c, int k, float *rgba_out) {
  if (!c || !rgba_out) return 1;
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->light_hist_n || !c->d_light_hist) FAIL(c, "smk_get_light_history: the last frame with shadows kept no history (option shadow_march 0?)");
  if (k < 0 || k >= c->light_hist_n) FAIL(c, "smk_get_light_history: slice %d outside 0..%d", k, c->light_hist_n - 1);
  HIPCHK(c, hipDeviceSynchronize());
  HIPCHK(c, hipMemcpy(rgba_out, c->d_light_hist + (size_t)k * c->light_hist_stride, (size_t)c->light_lb * c->light_lb * 16,
                      hipMemcpyDeviceToHost));
  return 0;
}
