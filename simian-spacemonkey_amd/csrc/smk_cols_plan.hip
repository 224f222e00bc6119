// smk_cols_plan.hip -- host-side planning of the column-stream kernel (smk_cols.hip): which frames
// it takes, the voxel-to-pixel projection, the column layout, the ring in LDS, the jobs, the side buffers and the launch;
// and its statistics (smk_get_stat "cols_*").
//
// smk_launch_cols runs the stages below in order.  Each reads what the earlier ones decided -- the frame (P), the launch
// parameters (Q), the plan (ColPlan) and the context's side buffers (ColsAux) -- and returns the reason (a refusal text,
// or hipErrorNotSupported and *why) where the frame must use another kernel.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "smk_cols.h"

// what the stages decide beside the launch parameters
struct ColPlan {
  int as, au, av;  // model axes of S (the principal axis), U and V
  int perm;        // layout: 0 S = z, 1 S = y, 2 S = x (ColsAux::lay)
  double dens;     // pixels per (u, v) cell of a slice, at the densest place
  double side_u, side_v;  // pixels under a cell's side faces along U / along V there, weighted (cols_density)
  double ds;       // slices a ray advances per plane, at least
  int cells_u, cells_v;   // cells of the stored box across the view (cols_cells: a pad column is no cell)
  int npos;               // slice positions along S to chunk (cols_cells)
  double slab;     // slices the thickest slab between two slice positions spans (the volume's outermost cells: below)
  int shape;       // workgroup shape (kColShapes)
  int vb;          // bytes per voxel
  size_t fixed;    // LDS beside the ring
  int njobs;
};

// ---- refusal: frames the kernel does not take, in this order
static const char *cols_refusal(const RenderParams &P, int dtype, int tf_mode) {
  if (P.zscene) return "scene depth";  // (smk_render_occluded: the ray-marchers take such frames)
  if (tf_mode < 0 || tf_mode > 2) return "no classification mode";
  if (tf_mode == 0 && (!P.tlut || P.tlut_size < 1)) return "no colour table";
  if (tf_mode == 1 && (!P.tf_vg || P.sv < 2 || P.sg < 2)) return "transfer function smaller than 2x2";
  if (tf_mode == 2 && (!P.tf3d || P.s3v < 1 || P.s3g < 1 || P.s3h < 1)) return "no 3-D table";
  if (P.pert_on) return "perturbation";
  if (P.blend == SMK_BLEND_BACK_TO_FRONT) return "back-to-front blend (columns stream front to back)";
  if (P.depth) return "first-hit depth requested";
  if (P.cplane_on) return "free clip plane";
  if (dtype == 1 && !P.n_in_w) return "4-channel f32 voxels";
  if (dtype == 2) return "u16 voxels (the column-stream kernel has no u16 instance)";
  if (P.rc.nplanes <= 0) return "no planes";
  for (int a = 0; a < 3; ++a) {
    if (P.D[a] < 2 || P.N[a] < 2) return "volume thinner than 2 voxels";
    if (!(P.lo[a] <= P.hin[a])) return "region is empty";
  }
  if (P.W > 16384 || P.H > 16384) return "viewport larger than 16384";
  return nullptr;
}

// ---- axes: the principal axis and marching direction from the central ray (every ray must share them), U and V, the
// stored box along them
static const char *cols_axes(const RenderParams &P, ColParams &Q, ColPlan &L) {
  const smk_raycoef &rc = P.rc;
  auto ray = [&](double fi, double fj, double A[3], double B[3]) {  // (at pixel position (fi, fj))
    host_ray_at(P, fi * (double)rc.pxs + (double)rc.pxl, fj * (double)rc.pys + (double)rc.pyl, A, B);
  };
  double Ac[3], Bc[3];
  ray(P.W * 0.5, P.H * 0.5, Ac, Bc);
  int as = 0;
  for (int a = 1; a < 3; ++a)
    if (fabs(Bc[a]) > fabs(Bc[as])) as = a;
  L.as = as;
  L.perm = as == 2 ? 0 : (as == 1 ? 1 : 2);
  L.au = L.perm == 2 ? 1 : 0;
  L.av = L.perm == 0 ? 1 : 2;
  const int dir = Bc[as] > 0 ? 1 : -1;
  double slope_u = 0, slope_v = 0;
  L.ds = fabs(Bc[as]);
  for (int c = 0; c < 4; ++c) {
    double A[3], B[3];
    ray((c & 1) ? P.W : 0.0, (c & 2) ? P.H : 0.0, A, B);
    if (!(B[as] * dir > 0) || fabs(B[as]) < 1e-12) return "rays do not share a marching direction";
    L.ds = std::min(L.ds, fabs(B[as]));
    slope_u = std::max(slope_u, fabs(B[L.au] / B[as]));
    slope_v = std::max(slope_v, fabs(B[L.av] / B[as]));
  }
  if (slope_u > 3.0 || slope_v > 3.0) return "view too oblique for the principal axis";
  Q.dir = dir;
  Q.Ou = P.O[L.au]; Q.Ov = P.O[L.av]; Q.Os = P.O[as];
  Q.Du = P.D[L.au]; Q.Dv = P.D[L.av]; Q.Ds = P.D[as];
  return nullptr;
}

// ---- cells: what the columns and the chunks divide.  A box of 8-byte voxels has even x and y extents; where the volume's
// own extent is odd the box ends in a pad voxel (index N, never sampled: the base cell of a clamped coordinate is at most
// N - 2).  The pad is no cell: a column, or a chunk, that held the pad's cell alone would have the volume's face as its
// whole box -- [N - 1, N - 1/2], whose samples have their base cell in the column (chunk) before it, which takes them as
// well -- every such sample twice, and fetched from one cell outside the column (found by the plan sweep,
// tests/test_gpu_cols_plans.py; counted in, the 129 cells of a box of 130 voxels in columns of 16 are eight columns and the
// pad).  Along U and V the pad cell is left out;
// along S it can only be left out where it is the LAST position, marching towards it (the kernel counts positions from the
// near end); marching away from it it is the first position of the first chunk, which has at least two.
static void cols_cells(const RenderParams &P, const ColParams &Q, ColPlan &L) {
  L.cells_u = std::max(std::min(Q.Du, P.N[L.au] - Q.Ou) - 1, 1);
  L.cells_v = std::max(std::min(Q.Dv, P.N[L.av] - Q.Ov) - 1, 1);
  L.npos = std::max((Q.dir > 0 ? std::min(Q.Ds, P.N[L.as] - Q.Os) : Q.Ds) - 1, 1);
}

static bool inv3(const double m[9], double o[9]) {
  const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  if (!(fabs(det) > 1e-300)) return false;
  const double id = 1.0 / det;
  o[0] = (m[4] * m[8] - m[5] * m[7]) * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  o[3] = (m[5] * m[6] - m[3] * m[8]) * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  o[6] = (m[3] * m[7] - m[4] * m[6]) * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
  return true;
}

// ---- projection: voxel -> continuous pixel (Q.Mx, My, Mw).  X + .5 = E' + tau d(px, py) with d = Bc + px Bx + py By (per
// unit of dtau) and A = E + tau0/dtau * B: (px, py, 1) tau/dtau = G^-1 (X - E), G = [Bx By Bc]
static const char *cols_projection(const RenderParams &P, ColParams &Q) {
  const smk_raycoef &rc = P.rc;
  const double G[9] = {rc.Bx[0], rc.By[0], rc.Bc[0], rc.Bx[1], rc.By[1], rc.Bc[1], rc.Bx[2], rc.By[2], rc.Bc[2]};
  double Gi[9];
  if (!inv3(G, Gi)) return "degenerate projection";
  const double k = (double)rc.tau0 / (double)rc.dtau;
  const double E[3] = {rc.Ac[0] - k * rc.Bc[0], rc.Ac[1] - k * rc.Bc[1], rc.Ac[2] - k * rc.Bc[2]};
  double row[3][4];
  for (int r = 0; r < 3; ++r) {
    for (int a = 0; a < 3; ++a) row[r][a] = Gi[3 * r + a];
    row[r][3] = -(Gi[3 * r] * E[0] + Gi[3 * r + 1] * E[1] + Gi[3 * r + 2] * E[2]);
  }
  // the sign of the homogeneous coordinate: positive in front of the eye (tau / dtau has dtau's sign)
  const double sgn = rc.dtau > 0 ? 1.0 : -1.0;
  for (int a = 0; a < 4; ++a) {
    Q.Mx[a] = (float)(sgn * (row[0][a] - (double)rc.pxl * row[2][a]) / (double)rc.pxs);
    Q.My[a] = (float)(sgn * (row[1][a] - (double)rc.pyl * row[2][a]) / (double)rc.pys);
    Q.Mw[a] = (float)(sgn * row[2][a]);
  }
  // scale so that w ~ 1 at the volume's centre (keeps the kernel's "w > 0" test well away from rounding)
  const double cx = 0.5 * P.N[0], cy = 0.5 * P.N[1], cz = 0.5 * P.N[2];
  const double wc = Q.Mw[0] * cx + Q.Mw[1] * cy + Q.Mw[2] * cz + Q.Mw[3];
  if (!(wc > 0)) return "volume centre behind the eye";
  for (int a = 0; a < 4; ++a) {
    Q.Mx[a] = (float)(Q.Mx[a] / wc);
    Q.My[a] = (float)(Q.My[a] / wc);
    Q.Mw[a] = (float)(Q.Mw[a] / wc);
  }
  return nullptr;
}

// ---- cell density: pixels per (u, v) cell of a slice at the volume's corners and centre (L.dens).  Every ray that is
// inside a column at one slice position wants a lane; with samples a slice or more apart (ds >= 1) those are, on average,
// at most the rays through the column's face, cells x rays per cell.  With samples closer than a slice every ray that
// crosses the slab between two slices has a sample in it, also the rays that enter or leave through the column's sides: a
// ray whose path through the slab spans p of a slice is inside with probability min(1, p / ds), p uniform on (0, 1) over
// the pixels under a side face, which adds (1 - ds) of those pixels, (t - ds) for a slab t slices thick -- L.side_u per cell
// along U, L.side_v along V (found
// by the feature fuzz: a two-slice volume seen obliquely from close by, tests/test_gpu_cols.py).
// The volume's outermost cells also take the half voxel beyond the outermost voxel centres (base cell = min((int)clamp(p,
// 0, N - 1), N - 2) of a p in [-.5, N - .5]): a column at a face is half a cell wider, one that spans the axis a whole
// cell, and the first and last slab are 1.5 slices thick (2 where there is one slab only).
// inside a column at one slice position wants a lane: cells x rays per cell (largest where the volume is nearest to the
// eye) must stay below the consumer lanes.
static const char *cols_density(const RenderParams &P, const ColParams &Q, ColPlan &L) {
  auto project = [&](double u, double v, double sc, double &x, double &y) -> bool {
    double X[3];
    X[L.au] = u; X[L.av] = v; X[L.as] = sc;
    const double w = Q.Mw[0] * X[0] + Q.Mw[1] * X[1] + Q.Mw[2] * X[2] + Q.Mw[3];
    if (!(w > 1e-9)) return false;
    x = (Q.Mx[0] * X[0] + Q.Mx[1] * X[1] + Q.Mx[2] * X[2] + Q.Mx[3]) / w;
    y = (Q.My[0] * X[0] + Q.My[1] * X[1] + Q.My[2] * X[2] + Q.My[3]) / w;
    return true;
  };
  double dens = 0, side_u = 0, side_v = 0;
  for (int c = 0; c < 9; ++c) {
    const double u = c == 8 ? 0.5 * P.N[L.au] : ((c & 1) ? P.N[L.au] - 0.5 : -0.5), v = c == 8 ? 0.5 * P.N[L.av] : ((c & 2) ? P.N[L.av] - 0.5 : -0.5),
                 sc = c == 8 ? 0.5 * P.N[L.as] : ((c & 4) ? P.N[L.as] - 0.5 : -0.5);
    // (the point one slice further on only has to be in front of the eye)
    double x0, y0, x1, y1, x2, y2, x3, y3;
    if (!project(u, v, sc, x0, y0) || !project(u + 1, v, sc, x1, y1) || !project(u, v + 1, sc, x2, y2) || !project(u, v, sc + 1, x3, y3))
      return "volume reaches behind the eye";
    dens = std::max(dens, fabs((x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)));
    side_u = std::max(side_u, fabs((x1 - x0) * (y3 - y0) - (x3 - x0) * (y1 - y0)));
    side_v = std::max(side_v, fabs((x2 - x0) * (y3 - y0) - (x3 - x0) * (y2 - y0)));
  }
  if (!(dens > 1e-9)) return "degenerate projection";
  L.dens = dens;
  L.slab = Q.Ds - 1 <= 1 ? 2.0 : 1.5;
  const double under = L.slab * std::max(0.0, 1.0 - L.ds / L.slab);
  L.side_u = under * side_u;
  L.side_v = under * side_v;
  return nullptr;
}

// ---- LDS budget: the workgroup shape (option cols_shape), the classification's tables in LDS and the fixed part of the
// workgroup's LDS -- ray list + entry positions + slot table + two histograms + control + alpha_H + occupancy bitmap
static const char *cols_lds_budget(const RenderParams &P, int dtype, int tf_mode, const ColsAux *aux, ColParams &Q, ColPlan &L) {
  L.shape = aux->opt_shape ? aux->opt_shape - 1 : 0;
  if (L.shape < 0 || L.shape >= COL_NSHAPES) return "no such workgroup shape";
  L.vb = dtype == 0 ? 8 : 16;
  const bool three = P.third_axis && P.tf_h;
  Q.use_ah = (tf_mode == 1 && three && P.nelts <= 3 && P.sv >= 2 && P.sv <= 1024) ? 1 : 0;
  Q.fast_tf = (tf_mode == 1 && (!three || Q.use_ah)) ? 1 : 0;
  const size_t occ_bytes = tf_mode == 1 ? (size_t)P.occ_roww * P.sg * 4 : tf_mode == 2 ? (size_t)P.occ_roww * P.s3g * 4 : 0;
  Q.use_occ = (P.tf_occ && occ_bytes > 0 && occ_bytes <= 16384 && (Q.fast_tf || tf_mode == 2)) ? 1 : 0;
  L.fixed = (size_t)COL_MAX_RAYS * 9 + (size_t)3 * (COL_MAX_CL + 4) * 4 + 32 * 4 + (Q.use_ah ? (size_t)P.sv * 4 : 0) + (Q.use_occ ? occ_bytes : 0) + 64;
  return nullptr;
}

// bytes of a column's slice image: (cw + 1) x (ch + 1) voxels, rounded up to 16
static size_t cols_slice_bytes(int cw, int ch, int vb) { return (((size_t)(cw + 1) * (ch + 1) * vb) + 15) & ~(size_t)15; }

// does a column of cw x ch cells fit: its rays in `fill` of the lanes at the densest place (the set-up checks every job
// exactly and reports, see the kernel), `slots` of its slice images in LDS, two slices in flight per loader within the
// vmcnt range
// rays inside a column of cw x ch cells at one slice position, at the densest place (cols_density): through its face, the
// column away from the volume's faces; and everything counted -- the outermost cells' half voxels, the side faces
static double cols_rays(const ColPlan &L, int cw, int ch) { return (double)cw * ch * L.dens; }
static double cols_rays_at_faces(const ColPlan &L, int cw, int ch) {
  const double w = cw + (cw >= L.cells_u ? 1.0 : 0.5), h = ch + (ch >= L.cells_v ? 1.0 : 0.5);
  return w * h * L.dens + w * L.side_u + h * L.side_v;
}

static bool cols_fits(const ColPlan &L, double fill, int cw, int ch, int slots) {
  const int lanes = kColShapes[L.shape].nw * 64;
  // (`fill` of the lanes leaves room for what the first count leaves out where columns are many cells wide and samples a
  //  slice or more apart; the second count must fit the lanes where they are not)
  if (cols_rays(L, cw, ch) > fill * lanes || cols_rays_at_faces(L, cw, ch) > lanes) return false;
  const size_t sb = cols_slice_bytes(cw, ch, L.vb);
  if (sb * slots + L.fixed > COL_LDS_CAP) return false;
  if ((sb + 1023) / 1024 * 2 > 63) return false;
  return true;
}

static void cols_free_layout(ColLayout &L) {
  if (L.d) (void)hipFree(L.d);
  L = ColLayout();
}

// columns as balanced divisions of the box: the squarest pair that fits `slots` slices, most cells first (least halo);
// false where none does
static bool cols_column_size(const ColPlan &L, double fill, int cells_u, int cells_v, int slots, int *bw, int *bh) {
  *bw = *bh = 0;
  double best = 1e300;
  for (int ncu = 1; ncu <= cells_u; ++ncu) {
    const int cw = (cells_u + ncu - 1) / ncu;
    if (cw > 255) continue;
    if (ncu > 1 && (cells_u + ncu - 2) / (ncu - 1) == cw) continue;  // (same width as with one column fewer)
    for (int ncv = 1; ncv <= cells_v; ++ncv) {
      const int ch = (cells_v + ncv - 1) / ncv;
      if (ch > 255) continue;
      if (ncv > 1 && (cells_v + ncv - 2) / (ncv - 1) == ch) continue;
      if (!cols_fits(L, fill, cw, ch, slots)) continue;
      const double over = (double)ncu * (cw + 1) * (double)ncv * (ch + 1) / ((double)cells_u * cells_v);
      if (over < best) { best = over; *bw = cw; *bh = ch; }
    }
  }
  return *bw != 0;
}

// ---- layout: the stored box in columns for this principal axis (ColsAux::lay[perm]), kept while its columns still suit
// the view, else sized, allocated (the other axes' layouts make room) and built.  Q: the layout's columns.
static hipError_t cols_layout(const RenderParams &P, ColParams &Q, const ColPlan &L, int dtype, const void *vox_native, ColsAux *aux,
                              const char **why, hipStream_t s) {
  ColLayout &LY = aux->lay[L.perm];
  const int lanes = kColShapes[L.shape].nw * 64;
  const int cells_u = L.cells_u, cells_v = L.cells_v;
  const double fill = (aux->opt_fill > 0 ? aux->opt_fill : 92) * 0.01;  // of the lanes, at the densest place
  bool reuse = LY.d && LY.Du == Q.Du && LY.Dv == Q.Dv && LY.Ds == Q.Ds && LY.src == vox_native && LY.vb == L.vb;
  if (reuse) {
    // an existing layout is kept while its columns fit the lanes and are not wastefully small for the view
    reuse = cols_fits(L, fill, LY.CW, LY.CH, 3) && (cols_rays(L, LY.CW, LY.CH) > 0.45 * lanes || (LY.CW >= cells_u && LY.CH >= cells_v));
  }
  if (!reuse) {
    int bw, bh;
    if (!cols_column_size(L, fill, cells_u, cells_v, aux->opt_ns ? aux->opt_ns : 6, &bw, &bh)) {
      *why = "no column size fits the lanes (view too close)";
      return hipErrorNotSupported;
    }
    const int ncu = (cells_u + bw - 1) / bw, ncv = (cells_v + bh - 1) / bh;
    const size_t sb = cols_slice_bytes(bw, bh, L.vb);
    const size_t bytes = (size_t)ncu * ncv * Q.Ds * sb;
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    if (LY.d) cols_free_layout(LY);
    if (bytes + ((size_t)2 << 30) > free_b + 0) {
      // make room: the other axes' layouts go first
      for (int k = 0; k < 3; ++k)
        if (k != L.perm) cols_free_layout(aux->lay[k]);
      (void)hipMemGetInfo(&free_b, &total_b);
      if (bytes + ((size_t)1 << 30) > free_b) { *why = "no memory for the column layout"; return hipErrorNotSupported; }
    }
    void *d = nullptr;
    if (hipMalloc(&d, bytes + 4096) != hipSuccess) { (void)hipGetLastError(); *why = "no memory for the column layout"; return hipErrorNotSupported; }
    LY.d = d; LY.bytes = bytes; LY.CW = bw; LY.CH = bh; LY.ncu = ncu; LY.ncv = ncv; LY.Du = Q.Du; LY.Dv = Q.Dv; LY.Ds = Q.Ds;
    LY.slice_bytes = (int)sb; LY.src = vox_native; LY.vb = L.vb;
    const size_t total = (size_t)ncu * ncv * Q.Ds * (size_t)(bw + 1) * (bh + 1);
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (total / 256 > 0x7fffffffull) { *why = "volume too large for the layout builder"; return hipErrorNotSupported; }
    hipError_t e = smk_cols_build(vox_native, dtype, L.perm, P.D, bw, bh, ncu, ncv, (int)sb, d, blocks, s);
    if (e != hipSuccess) return e;
    ++aux->builds;
  }
  Q.lay = (const char *)LY.d;
  Q.CW = LY.CW; Q.CH = LY.CH; Q.ncu = LY.ncu; Q.ncv = LY.ncv;
  Q.slice_bytes = LY.slice_bytes;
  return hipSuccess;
}

// ---- ring: the DMA instructions per slice, the slots in LDS (option cols_ns caps them), slices in flight per loader
// (cols_fly), the band wait (cols_wstep) and when a wave takes new rays (cols_take_min, cols_take_wait).
// The band wait is bounded by the ring: a consumer at position p waits for min(p + 2 + wstep, npos + 1) landed slices, the
// last of them load p + 1 + wstep, and a loader issues load r only while r - nslots < the slowest consumer's position <= p
// -- so that load is issued only where wstep <= nslots - 2.  A larger request (cols_wstep up to 7, whatever cols_ns says)
// would wait for a slice the ring cannot hold until the bounded spin gives up (status 1): it is clamped.
static const char *cols_ring(const ColsAux *aux, const ColPlan &L, ColParams &Q) {
  Q.n_ch = (Q.slice_bytes + 1023) / 1024;
  const int last_units = Q.slice_bytes / 16 - 64 * (Q.n_ch - 1);
  Q.last_mask = last_units >= 64 ? ~0ull : ((1ull << last_units) - 1ull);
  int nslots = (int)((COL_LDS_CAP - L.fixed) / (size_t)Q.slice_bytes);
  if (aux->opt_ns) nslots = std::min(nslots, aux->opt_ns);
  nslots = std::min(nslots, 12);
  if (nslots < 3) return "column slice does not fit LDS three times";
  Q.nslots = nslots;
  Q.maxfly = std::max(1, std::min(aux->opt_fly > 0 ? aux->opt_fly : 2, (nslots - 2) / kColShapes[L.shape].nl));
  while (Q.maxfly > 1 && Q.n_ch * Q.maxfly > 63) --Q.maxfly;  // (the counted vmcnt wait takes an immediate < 64)
  if (Q.n_ch > 63) return "column slice needs more than 63 DMA instructions";
  Q.wstep = std::min(aux->opt_wstep ? aux->opt_wstep - 1 : (nslots >= 7 ? 2 : nslots >= 5 ? 1 : 0), nslots - 2);
  Q.take_min = aux->opt_take_min > 0 ? aux->opt_take_min : 16;
  Q.take_wait = aux->opt_take_wait > 0 ? aux->opt_take_wait - 1 : 3;
  return nullptr;
}

// ---- chunks and keys: the slice positions (cols_cells) in equal chunks of at most 128 (option cols_chunk, 4..COL_MAX_CL);
// a segment key per column index along U and V and per chunk
static const char *cols_chunks(const ColsAux *aux, ColParams &Q, ColPlan &L) {
  const int npos_total = L.npos;
  int clmax = aux->opt_chunk ? std::min(aux->opt_chunk, COL_MAX_CL) : 128;
  clmax = std::max(clmax, 4);
  Q.nck = (npos_total + clmax - 1) / clmax;
  Q.CL = (npos_total + Q.nck - 1) / Q.nck;
  Q.nck = (npos_total + Q.CL - 1) / Q.CL;
  Q.nkeys = Q.ncu + Q.ncv + Q.nck - 2;
  Q.mask_words = (Q.nkeys + 63) / 64;
  if (Q.mask_words > 8) return "more than 512 segment keys";
  L.njobs = Q.ncu * Q.ncv * Q.nck;
  return nullptr;
}

// ---- side buffers: the segment layers and masks for W x H pixels, the job ticks, the developer counters
static hipError_t cols_side_buffers(const RenderParams &P, ColParams &Q, const ColPlan &L, ColsAux *aux, int *status_word, const char **why,
                                    hipStream_t s) {
  const size_t npix = (size_t)P.W * P.H;
  const size_t lay_bytes = (size_t)Q.nkeys * npix * 16;
  if (lay_bytes > aux->layers_cap) {
    if (aux->d_layers) (void)hipFree(aux->d_layers);
    aux->d_layers = nullptr; aux->layers_cap = 0;
    if (hipMalloc(&aux->d_layers, lay_bytes) != hipSuccess) { (void)hipGetLastError(); *why = "no memory for the segment layers"; return hipErrorNotSupported; }
    aux->layers_cap = lay_bytes;
  }
  const size_t mask_bytes = npix * Q.mask_words * 8;
  if (mask_bytes > aux->masks_cap || aux->masks_dirty) {
    if (mask_bytes > aux->masks_cap) {
      if (aux->d_masks) (void)hipFree(aux->d_masks);
      aux->d_masks = nullptr; aux->masks_cap = 0;
      if (hipMalloc(&aux->d_masks, mask_bytes) != hipSuccess) { (void)hipGetLastError(); *why = "no memory for the segment masks"; return hipErrorNotSupported; }
      aux->masks_cap = mask_bytes;
    }
    hipError_t e = hipMemsetAsync(aux->d_masks, 0, aux->masks_cap, s);
    if (e != hipSuccess) return e;
    aux->masks_dirty = false;
  }
  aux->mask_words_last = Q.mask_words;
  if (L.njobs > aux->ticks_cap) {
    if (aux->d_ticks) (void)hipFree(aux->d_ticks);
    aux->d_ticks = nullptr; aux->ticks_cap = 0;
    if (hipMalloc((void **)&aux->d_ticks, (size_t)L.njobs * 12) != hipSuccess) { (void)hipGetLastError(); *why = "no memory"; return hipErrorNotSupported; }
    aux->ticks_cap = L.njobs;
  }
  if (!aux->d_counts) {
    if (hipMalloc((void **)&aux->d_counts, 8 * 8) != hipSuccess) { (void)hipGetLastError(); *why = "no memory"; return hipErrorNotSupported; }
  }
  Q.layers = (float4 *)aux->d_layers;
  Q.masks = (unsigned long long *)aux->d_masks;
  Q.status = status_word;
  Q.status_tag = aux->status_tag;
  Q.job_ticks = aux->d_ticks;
  Q.counts = aux->want_counts ? aux->d_counts : nullptr;
  if (Q.counts) return hipMemsetAsync(aux->d_counts, 0, 64, s);
  return hipSuccess;
}

// ---- launch: the plan recorded for the statistics, the marching kernel's instance, then the resolve pass
static hipError_t cols_run(const RenderParams &P, ColParams &Q, const ColPlan &L, ColsAux *aux, int dtype, int tf_mode, int shade_kind,
                           const char **why, hipStream_t s) {
  aux->njobs_last = L.njobs;
  aux->cw_last = Q.CW; aux->ch_last = Q.CH; aux->nslots_last = Q.nslots; aux->shape_last = L.shape;
  aux->last_stream_bytes = (double)L.njobs / Q.nck * ((double)(Q.Ds - 1) + Q.nck) * Q.slice_bytes;
  const int plan[ColsAux::PLAN_FIELDS] = {Q.CW, Q.CH, Q.ncu, Q.ncv, Q.slice_bytes, Q.n_ch, (int)__builtin_popcountll(Q.last_mask),
                                          Q.nslots, Q.maxfly, Q.wstep, Q.take_min, Q.take_wait, Q.CL, Q.nck, Q.nkeys, Q.mask_words,
                                          L.shape, L.perm, Q.dir};
  memcpy(aux->plan_last, plan, sizeof plan);
  Q.ring_bytes = (int)std::max((size_t)Q.nslots * Q.slice_bytes, (size_t)COL_MAX_RAYS * 16);  // (set-up scratch: the unsorted rays)
  const size_t lds = (size_t)Q.ring_bytes + L.fixed;
  if (lds > COL_LDS_CAP) { *why = "column job does not fit LDS"; return hipErrorNotSupported; }
  if (aux->frame_ev0) {
    hipError_t e = hipEventRecord(aux->frame_ev0, s);
    if (e != hipSuccess) return e;
  }
  hipError_t e = smk_cols_march(P, Q, dtype, tf_mode, shade_kind, L.perm, L.shape, lds, L.njobs, s);
  if (e == hipErrorInvalidValue) { *why = "no column-stream instance for this mode"; return hipErrorNotSupported; }
  if (e != hipSuccess) return e;
  aux->masks_dirty = true;  // (until the resolve pass below has run; it clears what it reads)
  e = smk_cols_resolve((const float4 *)aux->d_layers, (unsigned long long *)aux->d_masks, Q.mask_words, (size_t)P.W * P.H, P.out,
                       P.blend == SMK_BLEND_MAX ? 1 : 0, s);
  if (e == hipSuccess) aux->masks_dirty = false;
  return e;
}

// plan + launch; hipErrorNotSupported (and *why) when the frame must use another kernel
hipError_t smk_launch_cols(RenderParams P, int dtype, int tf_mode, int shade_kind, const void *vox_native, ColsAux *aux, int *status_word,
                           const char **why, hipStream_t s) {
  ColParams Q;
  memset(&Q, 0, sizeof Q);
  ColPlan L = {};
  if ((*why = cols_refusal(P, dtype, tf_mode))) return hipErrorNotSupported;
  if (tf_mode == 0) shade_kind = 0;
  if ((*why = cols_axes(P, Q, L))) return hipErrorNotSupported;
  cols_cells(P, Q, L);
  if ((*why = cols_projection(P, Q)) || (*why = cols_density(P, Q, L)) ||
      (*why = cols_lds_budget(P, dtype, tf_mode, aux, Q, L)))
    return hipErrorNotSupported;
  hipError_t e = cols_layout(P, Q, L, dtype, vox_native, aux, why, s);
  if (e != hipSuccess) return e;
  if ((*why = cols_ring(aux, L, Q)) || (*why = cols_chunks(aux, Q, L))) return hipErrorNotSupported;
  if ((e = cols_side_buffers(P, Q, L, aux, status_word, why, s)) != hipSuccess) return e;
  return cols_run(P, Q, L, aux, dtype, tf_mode, shade_kind, why, s);
}

void smk_cols_free(ColsAux *aux) {
  for (int k = 0; k < 3; ++k) cols_free_layout(aux->lay[k]);
  if (aux->d_layers) (void)hipFree(aux->d_layers);
  if (aux->d_masks) (void)hipFree(aux->d_masks);
  if (aux->d_ticks) (void)hipFree(aux->d_ticks);
  if (aux->d_counts) (void)hipFree(aux->d_counts);
  *aux = ColsAux();
}

void smk_cols_drop_layouts(ColsAux *aux) {
  for (int k = 0; k < 3; ++k) cols_free_layout(aux->lay[k]);
}

// the fields of "cols_plan_<field>" in the order cols_run records them (ColsAux::plan_last; last_units: the lanes of the
// last DMA instruction's mask as the kernel gets it)
static const char *const kColsPlanFields[ColsAux::PLAN_FIELDS] = {"cw", "ch", "ncu", "ncv", "slice_bytes", "n_ch", "last_units", "nslots", "maxfly",
                                                                  "wstep", "take_min", "take_wait", "cl", "nck", "nkeys", "mask_words", "shape",
                                                                  "perm", "dir"};

// ---- statistics of the latest frame (smk_get_stat "cols_*"); these synchronise (the plan's fields do not)
int smk_cols_stat(smk_ctx *c, const char *name, double *value) {
  const ColsAux &A = c->cols;
  *value = 0.0;
  if (!strncmp(name, "cols_plan_", 10)) {  // host memory; 0 unless the latest frame was this kernel's
    for (int k = 0; k < ColsAux::PLAN_FIELDS; ++k)
      if (!strcmp(name + 10, kColsPlanFields[k])) {
        if (c->last_kernel == 4) *value = A.plan_last[k];
        return 0;
      }
    FAIL(c, "smk_get_stat: unknown name '%s'", name);
  }
  if (!strcmp(name, "cols_builds")) { *value = A.builds; return 0; }
  if (!strcmp(name, "cols_config")) { *value = A.cw_last | (A.ch_last << 8) | (A.nslots_last << 16) | (A.shape_last << 24); return 0; }
  if (!strcmp(name, "cols_jobs")) { *value = A.njobs_last; return 0; }
  if (!strcmp(name, "cols_stream_bytes")) { *value = A.last_stream_bytes; return 0; }
  if (!strcmp(name, "cols_job_ms_max") || !strcmp(name, "cols_job_ms_sum") || !strcmp(name, "cols_setup_ms_sum") || !strcmp(name, "cols_rays")) {
    const int nj = A.njobs_last, part = name[5] == 'j' ? 0 : name[5] == 's' ? 1 : 2;  // d_ticks: [3][nj] job, set-up ticks, rays
    if (c->last_kernel == 4 && A.d_ticks && nj > 0) {
      std::vector<unsigned> h((size_t)nj);
      if (read_back(c, h.data(), A.d_ticks + (size_t)nj * part, h.size())) return 1;
      double mx = 0, sum = 0;
      for (unsigned v : h) {
        mx = std::max(mx, (double)v);
        sum += v;
      }
      *value = part == 2 ? sum : (name[12] == 'm' ? mx : sum) * 1e-5;  // (100 MHz ticks)
    }
    return 0;
  }
  static const char *cn[8] = {"cols_samples", "cols_visible", "cols_slices", "cols_segments", "cols_iters", "cols_active_lanes", "cols_switch_iters", "cols_switch_lanes"};
  for (int k = 0; k < 8; ++k)
    if (!strcmp(name, cn[k])) {
      unsigned long long v = 0;
      if (A.d_counts && A.want_counts && read_back(c, &v, A.d_counts + k, 1)) return 1;
      *value = (double)v;
      return 0;
    }
  FAIL(c, "smk_get_stat: unknown name '%s'", name);
}
