// smk_slab_plan.hip -- host-side planning of the slice-ring kernel (smk_slab.hip): which frames it takes, its workgroup
// shape, the window and the ring in LDS, the tiles' weights, depth segments and the work-balanced schedule, and the
// launch.  DESIGN.md section 4 has the measurements behind every number.
//
// smk_launch_slab runs the stages below in order.  Each reads what the earlier ones decided -- the frame (P), the
// launch parameters (Q) and the context's side buffers (SlabAux) -- and returns the reason (hipErrorNotSupported) where
// the frame must use the gather kernel.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <vector>

#include "smk_slab.h"

// a ray's coefficients on the host, for planning: at a real-valued position (px, py) of the image plane, in double -- the
// kernels' float chains (smk_ray_AB) round differently by less than the planning's own slack
void host_ray_at(const RenderParams &P, double px, double py, double A[3], double B[3]) {
  const smk_raycoef &rc = P.rc;
  if (!P.sh.on) {
    for (int a = 0; a < 3; ++a) {
      A[a] = px * rc.Ax[a] + py * rc.Ay[a] + rc.Ac[a];
      B[a] = px * rc.Bx[a] + py * rc.By[a] + rc.Bc[a];
    }
    return;
  }
  const SmkShadowRays &sh = P.sh;  // frames with shadows: half-angle slices (smk_internal.h)
  const double nD = px * sh.nDx + py * sh.nDy + sh.nDc, tauA = sh.numA / nD, dtau = sh.dB / nD;
  for (int a = 0; a < 3; ++a) {
    const double D = px * sh.Dx[a] + py * sh.Dy[a] + sh.Dc[a];
    A[a] = sh.Ec[a] + tauA * D;
    B[a] = dtau * D;
  }
}
static void host_ray(const RenderParams &P, int i, int j, double A[3], double B[3]) {
  const smk_raycoef &rc = P.rc;
  const float px = fmaf((float)i + 0.5f, rc.pxs, rc.pxl), py = fmaf((float)j + 0.5f, rc.pys, rc.pyl);
  if (P.sh.on) {
    host_ray_at(P, px, py, A, B);
    return;
  }
  for (int a = 0; a < 3; ++a) {
    A[a] = fmaf(px, rc.Ax[a], fmaf(py, rc.Ay[a], rc.Ac[a]));
    B[a] = fmaf(px, rc.Bx[a], fmaf(py, rc.By[a], rc.Bc[a]));
  }
}

// ---- S-extent of (a tile's ray bundle between the first and the last sample plane) /\ (the region
// box), in voxel index coordinates.  The bundle is the pyramid section spanned by the rays through
// the tile's outer pixel EDGES (half a pixel beyond the corner pixels' centres, so a one-pixel-wide
// tile is not degenerate); rays are affine in the pixel coordinate, so every ray of the tile lies
// inside it.  Both bodies are convex: the extrema over the intersection sit on its vertices = the
// vertices of the box faces clipped by the pyramid's six planes + the pyramid's corners inside the
// box.  Corner rays alone do not bound this: all four may miss a volume that projects inside the
// tile, and a ray through a side face enters anywhere between the front and the back face.
namespace {
struct SlabVec { double v[3]; };

int slab_clip_polygon(const SlabVec *in, int n, const double pl[4], SlabVec *out) {  // keeps pl.(p,1) >= 0
  int m = 0;
  for (int k = 0; k < n; ++k) {
    const SlabVec &a = in[k], &b = in[(k + 1) % n];
    const double da = pl[0] * a.v[0] + pl[1] * a.v[1] + pl[2] * a.v[2] + pl[3];
    const double db = pl[0] * b.v[0] + pl[1] * b.v[1] + pl[2] * b.v[2] + pl[3];
    if (da >= 0) out[m++] = a;
    if ((da >= 0) != (db >= 0)) {
      const double t = da / (da - db);
      SlabVec c;
      for (int i = 0; i < 3; ++i) c.v[i] = a.v[i] + t * (b.v[i] - a.v[i]);
      out[m++] = c;
    }
  }
  return m;
}

// The common case without clipping: when the four corner rays enter the box through ONE face and leave it through ONE
// face (inside the sampled plane range), so does every ray between them -- the rays through a face form a convex set --
// and bundle /\ box is the hexahedron of the four entry and four exit points: its S-extent is theirs.  (A bundle that
// contains a box edge or vertex, or is cut by the first / last sample plane, goes the exact way above.)
static bool slab_bundle_slice_range_fast(const RenderParams &P, double fx0, double fy0, double fx1, double fy1, int as, double *smin,
                                         double *smax) {
  const smk_raycoef &rc = P.rc;
  const double fx[4] = {fx0, fx1, fx1, fx0}, fy[4] = {fy0, fy0, fy1, fy1};
  const double q0 = -0.5, q1 = (double)(rc.nplanes - 1) + 0.5, eps = 1e-3;
  int fin = -1, fout = -1;
  double mn = 1e300, mx = -1e300;
  for (int c = 0; c < 4; ++c) {
    const double px = fx[c] * (double)rc.pxs + (double)rc.pxl, py = fy[c] * (double)rc.pys + (double)rc.pyl;
    double A[3], B[3], te = -1e300, tx = 1e300;
    int ie = -1, ix = -1;
    host_ray_at(P, px, py, A, B);
    for (int a = 0; a < 3; ++a) {
      const double lo = (double)P.lo[a] - eps, hi = (double)P.hi[a] + eps;
      if (fabs(B[a]) < 1e-12) {
        if (A[a] < lo || A[a] > hi) return false;
        continue;
      }
      const double t1 = (lo - A[a]) / B[a], t2 = (hi - A[a]) / B[a];
      const double tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
      if (tn > te) { te = tn; ie = 2 * a + (t1 < t2 ? 0 : 1); }
      if (tf < tx) { tx = tf; ix = 2 * a + (t1 < t2 ? 1 : 0); }
    }
    if (!(te < tx) || te < q0 || tx > q1 || ie < 0 || ix < 0) return false;
    if (c == 0) { fin = ie; fout = ix; }
    else if (ie != fin || ix != fout) return false;
    const double se = A[as] + te * B[as], sx = A[as] + tx * B[as];
    mn = std::min(mn, std::min(se, sx));
    mx = std::max(mx, std::max(se, sx));
  }
  *smin = std::max(mn, (double)P.lo[as]);
  *smax = std::min(mx, (double)P.hi[as]);
  return true;
}

bool slab_bundle_slice_range_exact(const RenderParams &P, double fx0, double fy0, double fx1, double fy1, int as, double *smin,
                                   double *smax) {
  const smk_raycoef &rc = P.rc;
  const double fx[4] = {fx0, fx1, fx1, fx0}, fy[4] = {fy0, fy0, fy1, fy1};  // cyclic
  const double q0 = -0.5, q1 = (double)(rc.nplanes - 1) + 0.5;
  SlabVec F[4][2];
  double cen[3] = {0, 0, 0}, scale = 1.0;
  for (int c = 0; c < 4; ++c) {
    const double px = fx[c] * (double)rc.pxs + (double)rc.pxl, py = fy[c] * (double)rc.pys + (double)rc.pyl;
    double Ar[3], Br[3];
    host_ray_at(P, px, py, Ar, Br);
    for (int a = 0; a < 3; ++a) {
      const double A = Ar[a], B = Br[a];
      F[c][0].v[a] = A + q0 * B;
      F[c][1].v[a] = A + q1 * B;
      cen[a] += (F[c][0].v[a] + F[c][1].v[a]) / 8.0;
      scale = std::max(scale, std::max(fabs(F[c][0].v[a]), fabs(F[c][1].v[a])));
    }
  }
  double planes[6][4];
  int npl = 0;
  auto add_plane = [&](const SlabVec &a, const SlabVec &b, const SlabVec &c) {
    double e1[3], e2[3], n[4];
    for (int i = 0; i < 3; ++i) { e1[i] = b.v[i] - a.v[i]; e2[i] = c.v[i] - a.v[i]; }
    n[0] = e1[1] * e2[2] - e1[2] * e2[1];
    n[1] = e1[2] * e2[0] - e1[0] * e2[2];
    n[2] = e1[0] * e2[1] - e1[1] * e2[0];
    const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(len > 1e-12 * scale * scale)) return;  // degenerate: not clipping keeps a superset
    for (int i = 0; i < 3; ++i) n[i] /= len;
    n[3] = -(n[0] * a.v[0] + n[1] * a.v[1] + n[2] * a.v[2]);
    if (n[0] * cen[0] + n[1] * cen[1] + n[2] * cen[2] + n[3] < 0)
      for (int i = 0; i < 4; ++i) n[i] = -n[i];
    // every corner of the pyramid stays inside (fp slack, sides that are not exactly planar)
    double worst = 0;
    for (int c = 0; c < 4; ++c)
      for (int e = 0; e < 2; ++e)
        worst = std::min(worst, n[0] * F[c][e].v[0] + n[1] * F[c][e].v[1] + n[2] * F[c][e].v[2] + n[3]);
    n[3] += -worst + 1e-6 * scale;
    for (int i = 0; i < 4; ++i) planes[npl][i] = n[i];
    ++npl;
  };
  for (int c = 0; c < 4; ++c) add_plane(F[c][0], F[c][1], F[(c + 1) & 3][0]);
  add_plane(F[0][0], F[1][0], F[2][0]);
  add_plane(F[0][1], F[1][1], F[2][1]);

  const double eps = 1e-3;
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = (double)P.lo[a] - eps; hi[a] = (double)P.hi[a] + eps; }
  double mn = 1e300, mx = -1e300;
  for (int c = 0; c < 4; ++c)
    for (int e = 0; e < 2; ++e) {
      const double *p = F[c][e].v;
      if (p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2]) {
        mn = std::min(mn, p[as]);
        mx = std::max(mx, p[as]);
      }
    }
  for (int a = 0; a < 3; ++a)
    for (int side = 0; side < 2; ++side) {
      const int b = (a + 1) % 3, c = (a + 2) % 3;
      SlabVec poly[2][24];
      const double bb[4] = {lo[b], hi[b], hi[b], lo[b]}, cc[4] = {lo[c], lo[c], hi[c], hi[c]};
      for (int k = 0; k < 4; ++k) {
        poly[0][k].v[a] = side ? hi[a] : lo[a];
        poly[0][k].v[b] = bb[k];
        poly[0][k].v[c] = cc[k];
      }
      int n = 4, cur = 0;
      for (int k = 0; k < npl && n > 0; ++k) {
        n = slab_clip_polygon(poly[cur], n, planes[k], poly[cur ^ 1]);
        cur ^= 1;
      }
      for (int k = 0; k < n; ++k) {
        mn = std::min(mn, poly[cur][k].v[as]);
        mx = std::max(mx, poly[cur][k].v[as]);
      }
    }
  if (!(mn <= mx)) return false;
  *smin = std::max(mn, (double)P.lo[as]);
  *smax = std::min(mx, (double)P.hi[as]);
  return true;
}

bool slab_bundle_slice_range(const RenderParams &P, double fx0, double fy0, double fx1, double fy1, int as, double *smin,
                             double *smax) {
  static const int check = getenv("SMK_DEBUG_SCAN") ? atoi(getenv("SMK_DEBUG_SCAN")) : 0;  // (developer: 1 = compare the short way with the exact one, 2 = exact only)
  if (check != 2 && slab_bundle_slice_range_fast(P, fx0, fy0, fx1, fy1, as, smin, smax)) {
    if (!check) return true;
    double a = 0, b = 0;
    const bool ok = slab_bundle_slice_range_exact(P, fx0, fy0, fx1, fy1, as, &a, &b);
    if (!ok || fabs(a - *smin) > 5e-3 || fabs(b - *smax) > 5e-3)  // (the exact way pads its clipping planes by 1e-6 of the scene's scale)
      fprintf(stderr, "[smk] SCAN MISMATCH tile (%g,%g)-(%g,%g): fast [%.9g, %.9g] exact %d [%.9g, %.9g]\n", fx0, fy0, fx1, fy1, *smin, *smax, (int)ok, a, b);
    return true;
  }
  return slab_bundle_slice_range_exact(P, fx0, fy0, fx1, fy1, as, smin, smax);
}
}  // namespace
// developer (SMK_DEBUG_TIME): where the host's planning time goes -- this frame's scans; sums over 60 slice-ring frames
// of the scans, of all of it up to the launch and of the whole launcher
static struct {
  const bool on = getenv("SMK_DEBUG_TIME") != nullptr;
  double frame_scan = 0, scan = 0, planned = 0, whole = 0;
  int n = 0;
} slab_clock;
static double slab_now() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

// A stage's answer for a candidate workgroup shape that does not fit where a later candidate may: try the next one
// (SLAB_NEXT_BIG: the stream is too heavy for a small workgroup).  Any other non-null answer declines the frame.
static const char SLAB_NEXT[] = "next shape", SLAB_NEXT_BIG[] = "next shape, a big one";

// ---- the kernel instance of a frame on one workgroup shape (smk_slab.h; which keys are built: slab_inst_missing)
struct SlabShape { int tw, th, nl; };
static int slab_waves(SlabShape sh) { return (sh.tw / 8) * (sh.th / 8); }
static SlabInst slab_inst_for(const RenderParams &P, const SlabParams &Q, int dtype, int tf_mode, int shade_kind, SlabShape sh) {
  SlabInst k = {dtype, shade_kind, Q.perm, slab_waves(sh), sh.nl, tf_mode, false, false, P.sh.on != 0, P.zscene != nullptr, P.sh.on == 2};
  // developer diagnostics (option lockstep bits 2..64) live in separate instances of the plain f32 + R8k kernels under the
  // 2-D table only: compiled into the product kernels they cost SGPRs (spills) in every frame
  k.diag = (P.lockstep & ~1) != 0 && dtype == 1 && shade_kind == 1 && tf_mode == 1 && !k.shd && !k.occ;
  // the brick-flag code: where the shape has flags, always with scene depth (it is exact with no flags), never under the 1-D table
  k.br = k.diag || (tf_mode != 0 && (k.occ || Q.bricks));
  return k;
}
// A class of frames -- voxel type, scene depth, shadows and their look -- of which no shape, shading or table at all has an
// instance: why, else null.  (The gather kernel renders such frames.)
static const char *slab_class_missing(const RenderParams &P, int dtype) {
  const char *why = nullptr;
  for (int i = 0; i < SLAB_INST_KINDS / 3; ++i)
    for (int f = 0; f < 4; ++f) {  // (diag and br)
      SlabInst k = slab_inst_at(dtype * (SLAB_INST_KINDS / 3) + i, f);
      k.shd = P.sh.on != 0; k.occ = P.zscene != nullptr; k.nvl = P.sh.on == 2;
      if (!(why = slab_inst_missing(k))) return nullptr;
    }
  return why;
}

// ---- refusal: frames the kernel does not take, in this order (tests/test_gpu_fuzz.py tallies the reasons)
static const char *slab_refusal(const RenderParams &P, int dtype, int tf_mode, const SlabParams &Q) {
  const char *no_instance = slab_class_missing(P, dtype);
  if (tf_mode < 0 || tf_mode > 2) return "no classification mode";
  if (tf_mode == 0 && (!P.tlut || P.tlut_size < 1)) return "no colour table";
  if (tf_mode == 2 && (!P.tf3d || P.s3v < 1 || P.s3g < 1 || P.s3h < 1)) return "no 3-D table";
  if (P.pert_on) return "perturbation";
  // (back-to-front frames -- VolumeRenderer.cpp:590 -- are composited FRONT TO BACK here: "over" is associative, the slices
  //  stream one way; what changes is the association of the blend -- a few ulp per sample, as with depth segments -- and a
  //  saturated ray may stop.  Option kernel = 1 renders them in the reference's own order.)
  if (P.N[0] < 2 || P.N[1] < 2 || P.N[2] < 2) return "volume thinner than 2 voxels";
  if (dtype == 1 && !P.n_in_w) return "4-channel f32 voxels";
  if (dtype == 2 && no_instance) return no_instance;  // (u16 voxels: none for scene depth, none in the NV20 look)
  if (P.rc.nplanes <= 0) return "no planes";
  if (no_instance) return no_instance;  // (the NV20 look: none for scene depth)
  if (P.sh.on) {
    // frames with shadows: the component of a ray along the slice normal is affine in the pixel coordinate; where it keeps
    // its sign over the viewport's corners no ray runs parallel to the slices (the planning divides by it)
    double lo_n = 1e300, hi_n = -1e300;
    for (int c = 0; c < 4; ++c) {
      const double px = ((c & 1) ? (double)P.W : 0.0) * P.rc.pxs + P.rc.pxl, py = ((c & 2) ? (double)P.H : 0.0) * P.rc.pys + P.rc.pyl;
      const double nD = px * P.sh.nDx + py * P.sh.nDy + P.sh.nDc;
      lo_n = std::min(lo_n, nD);
      hi_n = std::max(hi_n, nD);
    }
    if (!(lo_n > 0 || hi_n < 0) || std::min(fabs(lo_n), fabs(hi_n)) < 1e-6 * std::max(fabs(lo_n), fabs(hi_n)))
      return "half-angle slices parallel to some eye ray";
  }
  if (Q.perm == 2 && !Q.vox) return "x-major copy unavailable";
  // (the free clip plane lives in the kernel's set-up: the kept samples of a ray are an interval of planes, see there; as a
  //  run-time test per sample in the consumers' loop it cost every frame WITHOUT a clip plane 4-5 % at 512^3 -- round 2)
  // an empty region (a clip plane outside a shard's box): the gather kernel's explicit comparisons
  // render it as nothing; the median-of-three membership test here needs lo <= hi
  for (int a = 0; a < 3; ++a)
    if (!(P.lo[a] <= P.hin[a])) return "region is empty";
  if (Q.Ds > 4096) return "more than 4096 slices";
  // u8 and u16 voxels are 8 B: the DMA moves 16-B units, so rows must start and end on even voxels
  if (dtype != 1 && ((Q.Du & 1) || (Q.strideV & 1) || (Q.strideS & 1))) return "odd U extent for 8-byte voxels";
  return nullptr;
}

// ---- axes: the principal axis S from the central ray, U and V, the marching direction, the stored box along them and
// the voxel layout that serves them.  Returns the central ray's |dS| per plane.
static double slab_axes(const RenderParams &P, const void *vox_native, const void *vox_xmajor, SlabParams &Q) {
  double Ac[3], Bc[3];
  host_ray(P, P.W / 2, P.H / 2, Ac, Bc);
  int as = 0;
  for (int a = 1; a < 3; ++a)
    if (fabs(Bc[a]) > fabs(Bc[as])) as = a;
  Q.as = as;
  if (as == 2) { Q.perm = 0; Q.au = 0; Q.av = 1; }
  else if (as == 1) { Q.perm = 1; Q.au = 0; Q.av = 2; }
  else { Q.perm = 2; Q.au = 1; Q.av = 2; }
  Q.dir = Bc[as] > 0 ? 1 : -1;
  Q.Ou = P.O[Q.au]; Q.Ov = P.O[Q.av]; Q.Os = P.O[as];
  Q.Du = P.D[Q.au]; Q.Dv = P.D[Q.av]; Q.Ds = P.D[as];
  if (Q.perm == 0) { Q.strideV = P.D[0]; Q.strideS = (long long)P.D[0] * P.D[1]; Q.vox = vox_native; }
  else if (Q.perm == 1) { Q.strideV = (long long)P.D[0] * P.D[1]; Q.strideS = P.D[0]; Q.vox = vox_native; }
  else { Q.strideV = P.D[1]; Q.strideS = (long long)P.D[1] * P.D[2]; Q.vox = vox_xmajor; }  // [x][z][y]
  return fabs(Bc[as]);
}

// ---- workgroup shapes: consumer waves are 8x8 pixel sub-tiles; NL loader waves.
//   light windows: 32x16 tile, 8+1 waves, two workgroups per CU
//   heavy windows (1024^3 f32 at a voxel per pixel): 24x32 tile, 12+4 waves, one per CU; the
//   tile is narrow along U so that a window row (tile + drift + pair) fits a 32-unit LDS pitch
// (one loader wave moves ~10 B/cycle at best, MI355X_MICROARCH.md 'ldsdma-fill'; a heavy
//  stream needs several per CU)
// Small-workgroup shape: 10 + 2 waves on 16x40 or 40x16 pixels, or 8 + 2 on 32x16 -- whichever needs the fewest DMA
// instructions per ray for THIS view (the window's width is rounded up to whole 128-byte units of LDS pitch, so the
// answer depends on the pose: cfg 3's gives 7 / 640, 8 / 640 and 6 / 512 rays, and 1.45 / 1.57 / 1.55 ms).  Two
// twelve-wave workgroups fill a CU's 24 wave slots at this kernel's 75-80 VGPRs; two ten-wave ones leave four idle.
// A probing pass sizes the candidates' windows (each scan is kept, see slab_scan), the real pass plans the winner.
// (a tie is won by the shape with the longer window rows, see the probe: same DMA count, rows twice as long; A/B on the cfg 3 frame turned
//  25 / 30 / 33 / 36 / 40 degrees, five alternations each: 0.611 / 0.577 / 0.614 / 0.636 / 0.625 ms against the narrow
//  shape's 0.606 / 0.614 / 0.627 / 0.654 / 0.641, tools/shape_ab.py)
static const SlabShape SLAB_CAND[3] = {{40, 16, 2}, {16, 40, 2}, {32, 16, 2}};
static const SlabShape SLAB_BIG_SHAPE = {32, 24, 4};
// option "tile" (developer): one shape, no choice.  The ids with a kernel instance (8+2, 10+2 or 12+4 waves); any other
// declines the frame.  tools/shape_ab.py and tools/shape_probe.py use 5, 20 and 21.
// (round 2: MORE loader waves -- 10+6 on 40x16 / 16x40 px, 8+8 on 32x16 / 16x32 -- on the 1024^3 frame: 5.10 / 7.76 /
//  6.30 / 7.21 ms against 4.33 for 12+4 on 32x24: the smaller tiles' extra fringe outweighs the issue slots)
static const struct { int id; SlabShape sh; } SLAB_TILE_OPTION[] = {
    {2, {24, 32, 4}}, {4, {32, 24, 4}}, {5, {32, 16, 2}}, {7, {16, 32, 2}}, {12, {48, 16, 4}}, {13, {16, 48, 4}}, {19, {48, 16, 4}}, {20, {40, 16, 2}}, {21, {16, 40, 2}}};

// ---- window scan of one tile shape: over every tile -- with `sparse`, every fourth tile row and column plus the
// borders -- the extent of the bundle's cross-section and its drift per slice (m[] = max_eu, max_ev, max_drift_u,
// max_drift_v), and the slices each tile streams (work: its schedule weight).  Returns the refusal or null.
// every ray must advance along S in the same direction and not too obliquely; window bound:
// bundle cross-section extent (corner rays of every tile) at the two S faces + drift over the
// two-slice interval a window covers + texel pair + eps
static const char *slab_scan(const RenderParams &P, const SlabParams &Q, bool sparse, SlabAux *aux, double m[4], std::vector<int> &work) {
  const int tw = Q.tw, th = Q.th, as = Q.as;
  const size_t nt = (size_t)P.ntx * P.nty;
  const double t0 = slab_clock.on ? slab_now() : 0;
  // The scan of all tiles below is a function of camera, region and tile shape alone; a frame of an unchanged
  // view reuses the last one (per tile ~0.3 us of double arithmetic: 0.65 ms for the 2048 tiles of a 1024^2
  // viewport -- hidden behind a 1.9 ms kernel, but not behind the 0.3 ms one of an eighth of the volume)
  struct ScanKey {
    smk_raycoef rc;
    int W, H, tw, th, as, au, av, dir, N[3], top[3];
    float lo[3], hi[3], hin[3];
    float sh[18];  // frames with shadows: the eye rays' coefficients (SmkShadowRays), else zeros
  } key;
  memset(&key, 0, sizeof key);
  key.rc = P.rc;
  if (P.sh.on) {
    const SmkShadowRays &h = P.sh;
    const float v[18] = {1.0f, h.Ec[0], h.Ec[1], h.Ec[2], h.Dc[0], h.Dc[1], h.Dc[2], h.Dx[0], h.Dx[1], h.Dx[2], h.Dy[0], h.Dy[1], h.Dy[2],
                         h.nDc, h.nDx, h.nDy, h.numA, h.dB};
    memcpy(key.sh, v, sizeof v);
  }
  key.W = P.W; key.H = P.H; key.tw = tw; key.th = th; key.as = as; key.au = Q.au; key.av = Q.av; key.dir = Q.dir;
  for (int a = 0; a < 3; ++a) { key.N[a] = P.N[a]; key.top[a] = P.top[a]; key.lo[a] = P.lo[a]; key.hi[a] = P.hi[a]; key.hin[a] = P.hin[a]; }
  int slot = -1;
  for (int k = 0; k < 4; ++k)
    if (aux->scan[k].key.size() == sizeof key && !memcmp(aux->scan[k].key.data(), &key, sizeof key) && aux->scan[k].work.size() == nt) slot = k;
  if (slot >= 0) {
    const SlabAux::Scan &scan = aux->scan[slot];
    for (int k = 0; k < 4; ++k) m[k] = scan.v[k];
    work = scan.work;
    aux->scan_slices = scan.slices;
    if (slab_clock.on) slab_clock.frame_scan += slab_now() - t0;
    return nullptr;
  }
  slot = aux->scan_next++ & 3;
  work.assign(nt, 1);
  // The rows of tiles are scanned by a few host threads (a pool the context keeps): ~0.13 us of double arithmetic per
  // tile is 0.27 ms for the 2048 tiles of a 1024^2 viewport on one thread -- as much as a shard's whole kernel when the
  // camera moves every frame.  Each thread keeps its own maxima and its own refusal; rows write disjoint tiles.
  struct Part { double eu = 0, ev = 0, du = 0, dv = 0; int slices = 0; const char *why = nullptr; };
  auto scan_rows = [&](int ty0, int ty1, Part &pt) {
    for (int tyi = ty0; tyi < ty1; ++tyi)
      for (int txi = 0; txi < P.ntx; ++txi) {
        if (sparse && !(((txi & 3) == 0 || txi == P.ntx - 1) && ((tyi & 3) == 0 || tyi == P.nty - 1))) continue;
        double cA[4][3], cB[4][3];
        for (int c = 0; c < 4; ++c) {
          int cx = std::min(txi * tw + ((c & 1) ? tw - 1 : 0), P.W - 1);
          int cy = std::min(tyi * th + ((c & 2) ? th - 1 : 0), P.H - 1);
          double *A = cA[c], *B = cB[c];
          host_ray(P, cx, cy, A, B);
          if (!(B[as] * Q.dir > 0) || fabs(B[as]) < 1e-12) { pt.why = "rays do not share a marching direction"; return; }
          double du = fabs(B[Q.au] / B[as]), dv = fabs(B[Q.av] / B[as]);
          // (3 voxels of drift per slice: close-ups with a wide frustum reach ~2.5 at the frame's edge and still
          //  run 2-3x faster here than on the gather kernel; the window bound below grows with the drift)
          if (du > 3.0 || dv > 3.0) { pt.why = "view too oblique for the principal axis"; return; }
          pt.du = std::max(pt.du, du);
          pt.dv = std::max(pt.dv, dv);
        }
        // the slices this tile can stream: S-extent of its ray bundle inside the region (exact for
        // the continuous bundle, see slab_bundle_slice_range)
        double smin_t, smax_t;
        if (!slab_bundle_slice_range(P, (double)(txi * tw), (double)(tyi * th), (double)std::min(txi * tw + tw, P.W),
                                     (double)std::min(tyi * th + th, P.H), as, &smin_t, &smax_t))
          continue;  // the bundle misses the region: nothing to stream
        work[(size_t)tyi * P.ntx + txi] = 16 + (int)(smax_t - smin_t);
        {  // the load indices of the tile (the kernel's npos + 1): base slices of the bundle's two ends, and the slice behind
          const double top = (double)(P.N[as] - 1);
          const int b0 = std::min((int)std::min(std::max(smin_t, 0.0), top), P.N[as] - 2), b1 = std::min((int)std::min(std::max(smax_t, 0.0), top), P.N[as] - 2);
          pt.slices = std::max(pt.slices, b1 - b0 + 2);
        }
        // cross-section of the bundle where THIS tile streams: it is linear in s (perspective), so
        // the two ends of the tile's own slice range bound it.  A sample at s reads slices floor(s)
        // and floor(s)+1, and the window of slice j covers s in [j-1, j+1] (stretched by half a
        // slice at the volume faces): 2.5 slices beyond the range.  (Bounding by the volume's S
        // faces instead costs 25-30 % window area at a voxel per pixel: rays are not inside the
        // volume where they are widest apart.)
        const double pad = 2.5 + 1e-2;
        const double se[2] = {std::max(-0.5, smin_t - pad), std::min((double)P.N[as] - 0.5, smax_t + pad)};
        for (int f = 0; f < 2; ++f) {
          double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
          for (int c = 0; c < 4; ++c) {
            double mm = (se[f] - cA[c][as]) / cB[c][as];
            double u = cA[c][Q.au] + cB[c][Q.au] * mm, v = cA[c][Q.av] + cB[c][Q.av] * mm;
            umin = std::min(umin, u); umax = std::max(umax, u);
            vmin = std::min(vmin, v); vmax = std::max(vmax, v);
          }
          pt.eu = std::max(pt.eu, umax - umin);
          pt.ev = std::max(pt.ev, vmax - vmin);
        }
      }
  };
  const int nthreads = (!sparse && P.nty >= 16 && P.ntx * P.nty >= 512) ? smk_host_pool_size() : 1;
  std::vector<Part> parts((size_t)std::max(nthreads, 1));
  if (nthreads <= 1) {
    scan_rows(0, P.nty, parts[0]);
  } else {
    smk_host_pool_run(nthreads, [&](int k) { scan_rows((int)((long long)P.nty * k / nthreads), (int)((long long)P.nty * (k + 1) / nthreads), parts[(size_t)k]); });
  }
  if (slab_clock.on) slab_clock.frame_scan += slab_now() - t0;
  m[0] = m[1] = m[2] = m[3] = 0;
  aux->scan_slices = 0;
  for (const Part &pt : parts) {
    if (pt.why) return pt.why;
    aux->scan_slices = std::max(aux->scan_slices, pt.slices);
    m[0] = std::max(m[0], pt.eu); m[1] = std::max(m[1], pt.ev);
    m[2] = std::max(m[2], pt.du); m[3] = std::max(m[3], pt.dv);
  }
  if (!sparse) {  // (a probe is sparse: only complete scans are kept)
    SlabAux::Scan &scan = aux->scan[slot];
    scan.key.assign(reinterpret_cast<const unsigned char *>(&key), reinterpret_cast<const unsigned char *>(&key) + sizeof key);
    for (int k = 0; k < 4; ++k) scan.v[k] = m[k];
    scan.work = work;
    scan.slices = aux->scan_slices;
  }
  return nullptr;
}

// ---- window and pitch of one tile shape from its scan: Wu x Wv voxels, the LDS pitch, the row groups and the DMA
// instructions per slice.  Returns the refusal, SLAB_NEXT or null.
static const char *slab_window(const RenderParams &P, SlabParams &Q, int dtype, bool big, const double m[4], bool last) {
  const int upv = dtype != 1 ? 2 : 1;  // (voxels per 16-byte unit: by voxel size)
  // a window spans s in [j-1, j+1] (2 slices of drift; 2.5 at a face; 3 where slice 1 of a
  // three-slice volume touches both); a coordinate range of extent e touches at most ceil(e) + 2
  // texels (pair included); eps for the fp32 chains
  const double span = P.N[Q.as] <= 3 ? 3.0 : 2.5;
  int Wu = (int)ceil(m[0] + span * m[2] + 2 * SLAB_EPS) + 2;
  int Wv = (int)ceil(m[1] + span * m[3] + 2 * SLAB_EPS) + 2;
  if (dtype != 1) Wu = ((Wu + 1) & ~1) + 2;  // even width, even alignment of the origin
  Wu = std::min(Wu, Q.Du);
  Wv = std::min(Wv, Q.Dv);
  if (Wu < 2 || Wv < 2) return "degenerate window";
  // fixed window shape: wu 16-byte units per row on an LDS pitch of the next multiple of 8 units
  // (128 B); the slot image is flat, so the (row, column) a DMA lane serves repeats every
  // per = wp / gcd(64, wp) chunks = rpg = 64 / gcd(64, wp) rows ("group")
  Q.wu = Wu / upv;
  Q.wv = Wv;
  if (Q.wu > 64) return last ? "window wider than one DMA chunk" : SLAB_NEXT;
  if (Q.Du > 2047 || Q.Dv > 2047) return "stored box wider than 2047 voxels across the view";
  // The pitch: the next multiple of 8 units -- or, where that gives fewer DMA instructions per slice, the next multiple
  // of 4 whose period is one the loaders know (per = 1, 3, 5, 7: pitches 12, 20, 28): a 17-unit row on a pitch of 20
  // (two groups of 16 rows x 5 chunks) instead of 24 (four groups of 8 rows x 3 chunks) is 10 instructions for 12, and a
  // ring that fits half a CU again.
  auto shape = [&](int wp, int &per, int &rpg, int &groups) {
    int g = 64, r = wp;
    while (r) { int t = g % r; g = r; r = t; }  // gcd(64, wp)
    per = wp / g;
    rpg = 64 / g;
    groups = (Q.wv + rpg - 1) / rpg;
  };
  int wp8 = (Q.wu + 7) & ~7, per8, rpg8, gr8;
  shape(wp8, per8, rpg8, gr8);
  Q.wp = wp8; Q.per = per8; Q.rpg = rpg8;
  const int wp4 = (Q.wu + 3) & ~3;
  if (wp4 != wp8) {
    int per4, rpg4, gr4;
    shape(wp4, per4, rpg4, gr4);
    if (per4 <= 7 && gr4 * per4 < gr8 * per8) { Q.wp = wp4; Q.per = per4; Q.rpg = rpg4; }
  }
  Q.groups = (Q.wv + Q.rpg - 1) / Q.rpg;
  // small workgroups: a window of whole row groups (its LDS image is that big anyway), see the loader's group loop
  if (!big && Q.groups * Q.rpg <= Q.Dv) Q.wv = Q.groups * Q.rpg;
  Q.chunks = Q.groups * Q.per;
  return nullptr;
}

// one candidate shape sized for this frame: its tiling, scan, window and pitch
static const char *slab_size_shape(RenderParams &P, SlabParams &Q, SlabShape sh, int dtype, bool sparse, bool last, SlabAux *aux,
                                   std::vector<int> &work) {
  Q.tw = sh.tw;
  Q.th = sh.th;
  P.ntx = (P.W + sh.tw - 1) / sh.tw;
  P.nty = (P.H + sh.th - 1) / sh.th;
  P.tiles_per_xcd = (P.ntx * P.nty + 7) / 8;
  double m[4];
  const char *why = slab_scan(P, Q, sparse, aux, m, work);
  return why ? why : slab_window(P, Q, dtype, slab_big(slab_waves(sh), sh.nl), m, last);
}

// ---- the probing pass: the candidate small shape with the fewest DMA instructions per ray (*best, -1 if no candidate's
// window fits), its window sized from a sparse scan.  Returns the refusal or null.
static const char *slab_probe(RenderParams P, SlabParams Q, int dtype, int tf_mode, int shade_kind, SlabAux *aux, int *best) {
  double best_score = 1e300;
  int best_wu = 0;
  std::vector<int> work;
  *best = -1;
  Q.bricks = P.bricks;  // (as slab_ring will have it)
  for (int ci = 0; ci < 3; ++ci) {
    const SlabShape sh = SLAB_CAND[ci];
    // (a shape whose workgroup has no kernel instance for this frame -- the ones left out because they would spill -- is passed over)
    if (slab_inst_missing(slab_inst_for(P, Q, dtype, tf_mode, shade_kind, sh))) continue;
    const char *why = slab_size_shape(P, Q, sh, dtype, true, false, aux, work);
    if (why == SLAB_NEXT) continue;
    if (why) return why;
    const int nw = slab_waves(sh);
    // (the ten-wave shape leaves four of a CU's wave slots idle: with the brick flags on it measures 0.83 ms on the cfg 3
    //  frame where the twelve-wave shapes take 0.59-0.61, although it needs the fewest DMA instructions per ray at some
    //  poses -- a camera turning through such a pose got 0.79 ms frames for 0.63.  It has to win by 40 % now.)
    const double score = (double)Q.chunks / (nw * 64) * (nw + sh.nl < 12 ? 1.4 : 1.0);
    // (a tie goes to the shape with the LONGER window rows -- the same DMA count in fewer, longer runs of memory: on the
    //  cfg 3 frame the wide shape, whose rows lie along the image's x there; a view turned a quarter about its axis has
    //  them along y)
    if (score < best_score || (score == best_score && Q.wu > best_wu)) { best_score = score; *best = ci; best_wu = Q.wu; }
  }
  return nullptr;
}

// ---- ring fit: the slice ring of the sized window in LDS beside the slice table, the control words and the
// classification tables -- slots, slices in flight per loader, band wait, publishing period.  Returns the refusal,
// SLAB_NEXT, SLAB_NEXT_BIG or null; *lds = the workgroup's LDS bytes.
static const char *slab_ring(const RenderParams &P, SlabParams &Q, SlabShape sh, int tf_mode, double ds, const SlabAux *aux, bool last,
                             size_t *lds) {
  const int nw = slab_waves(sh), nl = sh.nl;
  const bool big = slab_big(nw, nl);
  Q.slot_bytes = Q.chunks * 1024;  // (whole KiB: the kernel's slice-table entries keep their low three bits free for flags)
  // per-slice extents (and with them the table-occupancy bitmap) from four chunks per slice up:
  // re-measured with two slices in flight, 512^3 f32 1.66 -> 1.58 ms, 512^3 u8 1.72 -> 1.68,
  // 256^3 at 1024^2 1.72 -> 1.55 (the first threshold, 12 chunks, dated from five slices in flight)
  Q.mask_need = Q.chunks >= 4 ? 1 : 0;
  // loaders of one slice (see the kernel: NLG groups of LPG loaders)
  const int nlg = slab_loader_groups(nw, nl), lpg = nl / nlg;
  const int mych = (Q.groups + lpg - 1) / lpg * Q.per;  // most DMA instructions one loader issues per slice
  if (mych > 63) return last ? "window needs more than 63 DMA chunks per loader" : SLAB_NEXT;
  // light enough for this configuration?  otherwise try the next (heavier-duty) one
  if (!last && (double)Q.chunks * 1024.0 / (nw * 64) > 16.0 * nl) return SLAB_NEXT_BIG;
  Q.use_ah = (tf_mode == 1 && P.third_axis && P.nelts <= 3 && P.sv >= 2 && P.sv <= 2048) ? 1 : 0;
  if (tf_mode == 1 && (P.sv < 2 || P.sg < 2)) return "transfer function smaller than 2x2";
  const size_t occ_bytes = tf_mode == 1 ? (size_t)P.occ_roww * P.sg * 4 : tf_mode == 2 ? (size_t)P.occ_roww * P.s3g * 4 : 0;
  Q.fast_tf = (tf_mode == 1 && (!P.third_axis || Q.use_ah)) ? 1 : 0;
  // (measured: 5.99 -> 5.61 ms on 1024^3, where the texel gathers share the texture path with a
  //  heavy stream; no gain at 512^3, where the 8 KB are worth more as ring slots)
  Q.use_occ = ((Q.fast_tf || tf_mode == 2) && Q.mask_need && P.tf_occ && occ_bytes > 0 && occ_bytes <= 8192) ? 1 : 0;
  {  // brick flags (EMPTY LAYERS in the kernel): model-axis strides -> the kernel's (U, V, S)
    Q.bricks = (tf_mode == 1 || tf_mode == 2) ? P.bricks : nullptr;
    const int bst[3] = {1, P.nbr[0], P.nbr[0] * P.nbr[1]};
    Q.bsu = bst[Q.au];
    Q.bsv = bst[Q.av];
    Q.bss = bst[Q.as];
  }
  const size_t fixed = (size_t)Q.Ds * sizeof(SlabEnt) + (8 + 32) * 4 + 64 + (Q.use_ah ? (size_t)P.sv * 4 : 0) + (Q.use_occ ? occ_bytes : 0);
  // ring: as many slots as fit two workgroups per CU (small tiles) or one (big tiles)
  const size_t budget = big ? 158 * 1024 : 78 * 1024;
  if (budget <= fixed) return "slice table does not fit LDS";
  int ns = (int)((budget - fixed) / (size_t)Q.slot_bytes);
  if (ns > 24) ns = 24;
  // a wave holds ceil(slices per plane) + 1 slices while it works and the loaders want a few in flight
  const int band = (int)ceil(ds) + 2;
  if (ns < band + 2 && 158 * 1024 > fixed) {
    // the ring of a small workgroup does not fit half a CU: one workgroup per CU it is -- then
    // rather the big tile with 16 waves than this one with 10
    if (!last && budget < 158 * 1024) return SLAB_NEXT;
    ns = (int)((158 * 1024 - fixed) / (size_t)Q.slot_bytes);
    if (ns > band + 4) ns = band + 4;
  }
  if (aux->opt_ns >= 3 && ns > aux->opt_ns) ns = aux->opt_ns;  // (experiment knob: cap the ring)
  if (ns < 3) return last ? "window does not fit LDS" : SLAB_NEXT;
  Q.nslots = ns;
  // (the set-up keeps a 16-byte brick mask per layer of bricks in the ring's memory before the stream starts)
  if (Q.bricks && (size_t)ns * Q.slot_bytes < ((size_t)((Q.Ds - 1) >> SMK_BRICK_LOG2) + 1) * 16) Q.bricks = nullptr;
  // Slices a loader keeps in flight.  TWO: a loader publishes a slice as landed only when it stops
  // issuing and waits for the oldest one, so a deep issue window delays every consumer that polls
  // for that slice -- and two slices per loader already cover the memory latency (4 loaders x 2 x
  // ~7 KiB per CU).  Measured (frames per setting 5/4/3/2/1 on a 5-slot ring): 1024^3 f32 4.27 /
  // 4.19 / 4.03 / 3.84 / 4.36 ms; 512^3 f32 (12 slots) 1.81 at 12, 1.66 at 2-4, 1.80 at 1; 1024^3 u8
  // 3.54 -> 2.94 ms.
  // (small workgroups since their loaders take whole slices in turn: ONE slice in flight per loader -- the other
  //  loader's is in flight beside it; 1 / 2: cfg 3 1.42-1.44 / 1.45-1.46 ms, other poses and a 256^3 frame -0.3 to -3 %)
  Q.maxfly = std::max(1, std::min(std::min(ns, 63 / mych + 1), aux->opt_fly > 0 ? aux->opt_fly : (nlg > 1 && !big ? 1 : 2)));
  // a deep ring lets the whole band step together (every lane active); on a short one a wave that
  // waits for its whole band leaves the loaders nothing to overlap with (measured, 1024^3: 5 slots,
  // wstep 0 / 1 / 2 -> 5.5 / 5.8 / 6.8 ms)
  // (re-measured with two slices in flight per loader, 5 slots: wstep 0 / 1 / 2 -> 3.80 / 3.68 / 4.68 ms)
  Q.wstep = std::max(0, std::min((int)ceil(ds), ns - 4));
  if (aux->opt_T > 0) Q.wstep = std::max(0, std::min(aux->opt_T - 1, ns - 3));  // (experiment knob: slab_T = wstep + 1)
  // (small workgroups, 10 slots against a band of 4: every other turn 1.87 ms, every turn 1.90, every 4th / 8th 2.0 / 2.2)
  Q.pmask = ns >= 2 * band ? 1 : 0;
  *lds = (size_t)ns * Q.slot_bytes + fixed;
  if (getenv("SMK_DEBUG"))
    fprintf(stderr, "[smk] slice-ring plan: tile %dx%d, %d+%d waves, window %d units x %d rows (pitch %d units), %d chunks/slice, %d slots of %d B, table+ctl %zu B, LDS %zu B, band %d, wstep %d, pmask %d, maxfly %d\n",
            sh.tw, sh.th, nw, nl, Q.wu, Q.wv, Q.wp, Q.chunks, ns, Q.slot_bytes, fixed, *lds, band, Q.wstep, Q.pmask, Q.maxfly);
  return nullptr;
}

// ---- shape choice: the shape of option "tile"; or the small shape the probe ranks first (kept for the view, see
// below), the other small one, then the big one -- the first whose window and ring fit.  Leaves P and Q planned for
// that shape, its LDS bytes, and the tiles' weights from its scan.  Returns the refusal or null.
static const char *slab_choose_shape(RenderParams &P, SlabParams &Q, int dtype, int tf_mode, int shade_kind, double ds, SlabAux *aux, SlabShape &shape,
                                     size_t *lds, std::vector<int> &work) {
  SlabShape list[3] = {{32, 16, 2}, SLAB_BIG_SHAPE, SLAB_BIG_SHAPE};
  int n = 2;
  const bool choose = aux->opt_tile == 0;
  if (!choose) {
    const auto *t = std::find_if(std::begin(SLAB_TILE_OPTION), std::end(SLAB_TILE_OPTION), [&](const auto &o) { return o.id == aux->opt_tile; });
    if (t == std::end(SLAB_TILE_OPTION)) return "no kernel instance for this tile size";
    list[0] = t->sh;
    n = 1;
  }
  // The choice is kept while the view keeps its principal axis, direction and sizes (re-examined every 64 frames): a
  // camera that moves every frame must not pay the probe -- nor flip between two shapes of nearly equal score, which
  // would throw away the measured schedule weights of the tiling each time.  The probe itself scans every fourth tile
  // row and column plus the borders (its answer only ranks the shapes; the real pass sizes the winner's window fully).
  struct ShapeKey { int as, dir, W, H, dtype, N[3]; float lo[3], hi[3]; int nv20; } skey;  // (nv20: that look's candidates differ)
  memset(&skey, 0, sizeof skey);
  skey.nv20 = P.sh.on == 2 ? 1 : (dtype == 2 && shade_kind == 2 && tf_mode == 2) ? 2 : 0;  // (2: the frames of SLAB_U16_LEFT_OUT)
  skey.as = Q.as; skey.dir = Q.dir; skey.W = P.W; skey.H = P.H; skey.dtype = dtype;
  for (int a = 0; a < 3; ++a) { skey.N[a] = P.N[a]; skey.lo[a] = P.lo[a]; skey.hi[a] = P.hi[a]; }
  const bool shape_known = choose && aux->shape_key.size() == sizeof skey && !memcmp(aux->shape_key.data(), &skey, sizeof skey) &&
                           aux->shape_choice >= 0 && ++aux->shape_age < 64;
  int best = shape_known ? aux->shape_choice : -1;
  const char *why = choose && !shape_known ? slab_probe(P, Q, dtype, tf_mode, shade_kind, aux, &best) : nullptr;
  if (why) return why;
  int alt = -1;  // the other small shape: tried before the big workgroup where the chosen one turns out not to fit
  if (best >= 0) {
    // (the probe sizes windows from a sparse scan and can rank a shape by a window it will not get: near a pitch step the
    //  real window of the narrow tile is half as big again, its ring no longer fits half a CU -- a turning camera then
    //  rendered 60 frames in a row on the big workgroup, 0.72 ms, where the other small shape takes 0.63)
    alt = best == 0 ? 1 : 0;
    list[0] = SLAB_CAND[best];
    list[1] = SLAB_CAND[alt];
    list[2] = SLAB_BIG_SHAPE;
    n = 3;
    if (!shape_known) {
      aux->shape_key.assign(reinterpret_cast<const unsigned char *>(&skey), reinterpret_cast<const unsigned char *>(&skey) + sizeof skey);
      aux->shape_choice = best;
      aux->shape_age = 0;
    }
  }
  for (int ci = 0; ci < n; ++ci) {
    shape = list[ci];
    const bool last = ci + 1 == n;
    why = slab_size_shape(P, Q, shape, dtype, false, last, aux, work);
    // (a kept shape is probed again the moment its own window changes size -- a narrow tile's window row crosses a pitch
    //  step of 8 units within a degree or two of a turning camera, its DMA count jumps by half, its ring no longer fits
    //  half a CU and the frames fall to the big workgroup: 0.72 ms where the other small shape takes 0.63 -- not only
    //  every 64 frames)
    if (!why && choose && best >= 0 && ci == 0) {
      if (shape_known && aux->shape_chunks != Q.chunks) aux->shape_age = 64;
      if (!shape_known) aux->shape_chunks = Q.chunks;
    }
    if (!why) why = slab_ring(P, Q, shape, tf_mode, ds, aux, last, lds);
    const char *missing = why ? nullptr : slab_inst_missing(slab_inst_for(P, Q, dtype, tf_mode, shade_kind, shape));
    if (missing) why = last ? missing : SLAB_NEXT;  // (passed over, as in the probe)
    if (why == SLAB_NEXT_BIG && alt >= 0 && ci == 0) ci = 1;  // (a stream this heavy is too heavy for the other small shape as well: the big one next)
    if (why == SLAB_NEXT || why == SLAB_NEXT_BIG) continue;
    if (why) return why;
    if (choose && alt >= 0 && ci == 1) {  // the alternative shape it is: kept from the next frame on
      aux->shape_choice = alt;
      aux->shape_chunks = Q.chunks;
      aux->shape_age = 0;
    }
    return nullptr;
  }
  return "no configuration fits";
}

// ---- measured weights: the previous frame's per-tile workgroup durations, when they are of this very tiling and
// marching direction (tsig), replace the geometric estimate in work[].  (The geometric estimate -- slices streamed --
// misses what consumers cost: on 1024^3 the XCDs holding the image's top and bottom rows ran 1.6x longer per slice
// than the central ones and the frame waited for them.)  Also (re)allocates the buffers the kernel writes them to.
static hipError_t slab_measured_weights(SlabAux *aux, long long tsig, int nt, std::vector<int> &work, SlabParams &Q) {
  ++aux->ticks_age;
  if (aux->ticks_pending && aux->ticks_stale && hipEventQuery(aux->ticks_ev) == hipSuccess) {  // (of another time step)
    aux->ticks_pending = aux->ticks_stale = false;
  }
  if (aux->ticks_pending && hipEventQuery(aux->ticks_ev) == hipSuccess) {  // a copy has come back
    // (adopted at once for a new tiling, refined after 4, 8 and 16 frames -- a new order changes
    //  who runs beside whom and with it the durations -- then every 32 frames: durations of a
    //  steady view barely move, and every new table is an upload and a host touch of the stream)
    const bool fresh = aux->ticks_good_sig != aux->ticks_pending_sig;
    const int due = aux->ticks_adopted < 3 ? (4 << aux->ticks_adopted) : 32;
    if (fresh || aux->ticks_age >= due) {
      if (fresh || (int)aux->ticks_good.size() != aux->ticks_pending_n) {
        aux->ticks_good.assign(aux->h_ticks, aux->h_ticks + aux->ticks_pending_n);
        aux->ticks_adopted = 0;
      } else {
        // damped: half the old weight, half the new measurement.  (Workgroups of a few tens of microseconds -- an
        // opaque table -- measure mostly who ran beside them: averaged, the schedule oscillated between two plans,
        // 0.11 and 0.20 ms for the same frame; there the SHORTEST duration seen is the tile's own cost.)
        unsigned longest_new = 0;
        for (int t = 0; t < aux->ticks_pending_n; ++t) longest_new = std::max(longest_new, aux->h_ticks[t]);
        for (int t = 0; t < aux->ticks_pending_n; ++t)
          aux->ticks_good[t] = longest_new < 10000u ? (aux->h_ticks[t] ? std::min(std::max(aux->ticks_good[t], 1u), aux->h_ticks[t]) : aux->ticks_good[t])
                                                    : (aux->ticks_good[t] + aux->h_ticks[t] + 1) / 2;
        ++aux->ticks_adopted;
      }
      aux->ticks_good_sig = aux->ticks_pending_sig;
      aux->ticks_age = 0;
      // the pieces' own durations, and the cuts they were measured under (DEPTH SEGMENTS: the next cuts come from them)
      if (aux->h_pticks && (int)aux->cuts_pending.size() == aux->ticks_pending_n * 10) {
        aux->pticks_good.assign(aux->h_pticks, aux->h_pticks + (size_t)aux->ticks_pending_n * 8);
        aux->cuts_good = aux->cuts_pending;
      }
      aux->recut = true;
    }
    aux->ticks_pending = false;
  }
  (void)hipGetLastError();
  if (aux->ticks_good_sig == tsig && (int)aux->ticks_good.size() == nt) {
    for (int t = 0; t < nt; ++t)
      if (aux->ticks_good[t] > 0) work[t] = (int)std::min<unsigned>(aux->ticks_good[t], 1u << 30);
  }
  if (nt > aux->ticks_cap) {
    if (aux->ticks_pending) (void)hipEventSynchronize(aux->ticks_ev);
    aux->ticks_pending = aux->ticks_stale = false;
    if (aux->d_ticks) (void)hipFree(aux->d_ticks);
    if (aux->h_ticks) (void)hipHostFree(aux->h_ticks);
    if (aux->d_pticks) (void)hipFree(aux->d_pticks);
    if (aux->h_pticks) (void)hipHostFree(aux->h_pticks);
    aux->d_ticks = aux->h_ticks = aux->d_pticks = aux->h_pticks = nullptr;
    aux->ticks_cap = 0;
    hipError_t e = hipMalloc((void **)&aux->d_ticks, (size_t)nt * 20);
    if (e == hipSuccess) e = hipMemset(aux->d_ticks, 0, (size_t)nt * 20);
    if (e == hipSuccess) e = hipHostMalloc((void **)&aux->h_ticks, (size_t)nt * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void **)&aux->d_pticks, (size_t)nt * 32);
    if (e == hipSuccess) e = hipMemset(aux->d_pticks, 0, (size_t)nt * 32);
    if (e == hipSuccess) e = hipHostMalloc((void **)&aux->h_pticks, (size_t)nt * 32, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    aux->ticks_cap = nt;
  }
  if (!aux->ticks_ev) {
    hipError_t e = hipEventCreateWithFlags(&aux->ticks_ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  Q.tile_ticks = aux->d_ticks;
  Q.piece_ticks = aux->d_pticks;
  Q.ntiles = nt;
  aux->ticks_n_last = nt;
  return hipSuccess;
}

// A time-step switch (smk_timesteps.hip): the durations were measured on another volume, whose empty space is not this
// one's.  The next frames plan from the geometric estimate again, uncut, exactly as a fresh context's first frame does; the
// geometry scans and the chosen tile shape (camera and sizes alone) are kept.
void smk_slab_forget_measurements(SlabAux *aux) {
  aux->ticks_good.clear();
  aux->ticks_good_sig = -1;
  aux->ticks_adopted = 0;
  aux->ticks_stale = aux->ticks_pending;
  aux->pticks_good.clear();
  aux->cuts_good.clear();
  aux->cuts.clear();
  aux->cuts_sig = -1;
  aux->cuts_engaged = false;
  aux->recut = true;
}

// every buffer and event of the context's slice-ring side (smk_destroy); the status ring and d_diag are made by the frame
// driver (smk_frame.hip), the rest here
void smk_slab_free(SlabAux *aux) {
  for (void *p : {(void *)aux->d_diag, (void *)aux->d_order, (void *)aux->d_pticks, aux->d_seg, (void *)aux->d_trace, (void *)aux->d_ticks})
    if (p) (void)hipFree(p);
  for (void *p : {(void *)aux->h_status, (void *)aux->h_pticks, (void *)aux->h_ticks, (void *)aux->h_order[0], (void *)aux->h_order[1],
                  (void *)aux->h_order[2], (void *)aux->h_order[3]})
    if (p) (void)hipHostFree(p);
  for (hipEvent_t e : {aux->order_ev[0], aux->order_ev[1], aux->order_ev[2], aux->order_ev[3], aux->ticks_ev})
    if (e) (void)hipEventDestroy(e);
}

// ---- depth-segment cuts (aux->cuts)
// DEPTH SEGMENTS: how many workgroups render each tile.  From MEASURED durations only (the geometric estimate says
// nothing about what a tile's samples cost): a tile longer than half the mean load of a workgroup slot is cut so that
// no piece is; tiles under 60 us are never cut (a segment costs its own set-up, ~13 us).  Small scenes therefore run
// unsplit, bit-identical to the gather kernel; option "slab_split" 1 turns it off, 2.. forces that many everywhere.
// cuts[t] = {pieces K, cut_0 = 0, ..., cut_K = 255}: the tile's slice positions in 255ths
static void slab_cut_segments(SlabAux *aux, const std::vector<int> &work, int nt, long long tsig, int opt_split, bool big) {
  const bool measured = aux->ticks_good_sig == tsig && (int)aux->ticks_good.size() == nt;
  if ((int)aux->cuts.size() != nt * 10 || aux->cuts_split != opt_split || aux->cuts_sig != tsig) {
    aux->cuts.assign((size_t)nt * 10, 0);
    for (int t = 0; t < nt; ++t) { aux->cuts[(size_t)t * 10] = 1; aux->cuts[(size_t)t * 10 + 2] = 255; }
    aux->cuts_split = opt_split;
    aux->cuts_sig = tsig;
    aux->recut = true;
  }
  if (aux->recut) {
    aux->recut = false;
    auto equal_cuts = [&](int t, int K) {
      unsigned char *c = &aux->cuts[(size_t)t * 10];
      c[0] = (unsigned char)K;
      for (int k = 0; k <= K; ++k) c[1 + k] = (unsigned char)(255 * k / K);
    };
    if (opt_split >= 2) {
      for (int t = 0; t < nt; ++t) equal_cuts(t, std::min(opt_split, 8));
    } else if (opt_split == 0 && measured) {
      long long total = 0;
      for (int t = 0; t < nt; ++t) total += work[t];
      const double wg_slots = 256.0 * (big ? 1 : 2);
      // a piece should take about half the mean load of a workgroup slot, never under 60 us (a piece costs its own
      // set-up, ~13 us); frames whose slots carry under 50 us each -- small scenes -- are not cut at all
      // ... and only frames whose longest tile stands well above the mean load of a slot: where the slots' summed load is
      // the bound (cfg 3 on one GPU: longest tile 0.52 ms, mean load 0.49 ms, frame 0.61 ms with every tile cut in two --
      // 0.62 uncut) pieces only add their set-up; on a shard of 1/8 of that volume (longest 0.24, mean 0.08) they are the gain
      const double mean_load = (double)total / wg_slots;
      double longest_tile = 0;
      for (int t = 0; t < nt; ++t) longest_tile = std::max(longest_tile, (double)work[t]);
      const double piece = std::max(0.75 * mean_load, 6000.0);  // 100 MHz ticks
      bool big_frame = mean_load >= 5000.0 && longest_tile > 1.5 * mean_load;
      if (aux->cuts_engaged && mean_load >= 5000.0 && longest_tile > 1.2 * mean_load) big_frame = true;  // (hysteresis)
      aux->cuts_engaged = big_frame;
      const bool have_pieces = (int)aux->pticks_good.size() == nt * 8 && (int)aux->cuts_good.size() == nt * 10;
      for (int t = 0; t < nt; ++t) {
        unsigned char *c = &aux->cuts[(size_t)t * 10];
        int Kw = (big_frame && (double)work[t] > 1.25 * piece) ? (int)std::min(8.0, ceil((double)work[t] / piece)) : 1;
        if (big_frame && c[0] >= 2 && Kw >= 1 && abs(Kw - (int)c[0]) <= 1 && (double)work[t] > piece) Kw = c[0];  // (a tile keeps its count while the wish is a neighbour of it)
        if (Kw == 1) { equal_cuts(t, 1); continue; }
        // the pieces this tile was last measured in: work per 255th of depth, piecewise constant
        const unsigned char *g = have_pieces ? &aux->cuts_good[(size_t)t * 10] : nullptr;
        const int Kg = g ? g[0] : 1;
        if (!g || Kg < 2) {
          if (c[0] != Kw) equal_cuts(t, Kw);
          continue;
        }
        double d[8], tot = 0, longest = 0;
        for (int k = 0; k < Kg; ++k) {
          d[k] = std::max(1.0, (double)aux->pticks_good[(size_t)t * 8 + k] - 1300.0);  // (less the piece's own set-up)
          tot += d[k];
          longest = std::max(longest, d[k]);
        }
        const bool same = !memcmp(g, c, 10);
        if (same && Kg == Kw && longest <= 1.3 * tot / Kg) continue;  // balanced enough: keep (no flip-flopping)
        // new cuts: equal shares of the measured cumulative work
        unsigned char nc[10] = {(unsigned char)Kw, 0};
        int k = 0;
        double acc = 0;  // work before piece k
        for (int j = 1; j < Kw; ++j) {
          const double want = tot * j / Kw;
          while (k < Kg - 1 && acc + d[k] < want) acc += d[k++];
          const double f = d[k] > 0 ? (want - acc) / d[k] : 0.5;
          int x = (int)lround(g[1 + k] + f * (g[2 + k] - g[1 + k]));
          x = std::max(x, (int)nc[j] + 1);
          x = std::min(x, 255 - (Kw - j));
          nc[1 + j] = (unsigned char)x;
        }
        nc[1 + Kw] = 255;
        memcpy(c, nc, 10);
      }
    } else {
      for (int t = 0; t < nt; ++t) equal_cuts(t, 1);
    }
  }
}

// ---- schedule: the workgroup of every block {tile | piece << 20 | pieces << 26, cuts}, eight XCD lists interleaved
// (block b runs on XCD b % 8, in order of b), then the list of split tiles for the merge pass (tile | pieces << 20) and
// their number.  The same weights and cuts give the same schedule (aux->plan_*): planning stays off the frame path.
static void slab_schedule(const RenderParams &P, SlabAux *aux, const std::vector<int> &work, int slots, std::vector<int2> &order) {
  const int nt = P.ntx * P.nty;
  if (aux->plan_slots == slots && aux->plan_work == work && aux->plan_cuts == aux->cuts && !aux->plan_order.empty()) {
    order = aux->plan_order;
    return;
  }
  std::vector<unsigned char> ksplit((size_t)nt, 1);
  for (int t = 0; t < nt; ++t) ksplit[t] = aux->cuts[(size_t)t * 10];
  // a piece's weight: its own measured duration when it was measured under these very cuts, else an equal share
  auto piece_weight = [&](int t, int k) -> int {
    const unsigned char *c = &aux->cuts[(size_t)t * 10];
    if ((int)aux->pticks_good.size() == nt * 8 && (int)aux->cuts_good.size() == nt * 10 && !memcmp(&aux->cuts_good[(size_t)t * 10], c, 10) &&
        aux->pticks_good[(size_t)t * 8 + k] > 0)
      return (int)std::min<unsigned>(aux->pticks_good[(size_t)t * 8 + k], 1u << 30);
    return work[t] / std::max<int>(c[0], 1);
  };
  // DEALT (round 3; it replaced contiguous runs of the image per XCD): tiles in order of falling weight, each to the XCD
  // that carries the least so far -- every XCD gets the same mix of long and short workgroups.  The dispatcher hands
  // blocks out in index order, block b to XCD b % 8, and a block whose XCD has no free slot holds back every block
  // behind it: the XCDs' lists advance in step, entry k of all eight together.  With a contiguous run of the image
  // per XCD the lists differ (166-240 tiles, the centre's runs hold more long tiles than an XCD has slots: two of
  // them must share a slot) and slots stood idle for a mean 10 us per turnover while work was pending elsewhere
  // (tools/timeline.py).  Dealt: cfg 3 0.609 -> 0.587 ms, the 1024^3 frame 1.176 -> 1.109; with every slice streamed
  // (equal tiles) no change.
  // What is dealt is a BLOCK of neighbouring tiles, not a single tile: neighbours
  // weigh about the same, so they also sit next to each other in their XCD's list and stream the same slices at
  // about the same time -- the window fringes they share are then fetched once per block and hit in that XCD's L2.
  // Single tiles scatter every tile's neighbours over the other seven XCDs: HBM-side traffic of the cfg 3 frame
  // 1.18 -> 1.46 GB (2 x 2 blocks: 1.31), of the north star with every slice streamed 22.4 -> 24.0 GB (4 x 4: 22.2).
  // Block size: 2 x 2 tiles where the tiles' weights differ (brick flags on: bigger blocks deal the work coarser --
  // measured 4 x 4: cfg 3 0.595 -> 0.604 ms, the 1024^3 frame 1.110 -> 1.136), 4 x 4 where they are nearly equal
  // (every slice streamed: 4.035 -> 4.01 ms and the traffic of the contiguous runs, 22.2 GB).
  std::vector<std::vector<int>> run(8);
  std::vector<int> ws;
  ws.reserve((size_t)nt);
  for (int t = 0; t < nt; ++t)
    if (work[t] > 0) ws.push_back(work[t]);
  std::sort(ws.begin(), ws.end());
  // "nearly equal": the heavier half of the tiles within 1.25 x of one another (95th percentile against the median;
  // the tiles along the volume's silhouette are short whatever the table)
  const bool even = ws.size() >= 16 && (long long)ws[ws.size() * 95 / 100] * 4 <= (long long)ws[ws.size() / 2] * 5;
  const int SLAB_DEAL_W = even ? 4 : 2, SLAB_DEAL_H = even ? 4 : 2;
  const int gbx = (P.ntx + SLAB_DEAL_W - 1) / SLAB_DEAL_W, gby = (P.nty + SLAB_DEAL_H - 1) / SLAB_DEAL_H;
  std::vector<long long> gw((size_t)gbx * gby, 0);
  for (int t = 0; t < nt; ++t) gw[(size_t)((t / P.ntx) / SLAB_DEAL_H) * gbx + (t % P.ntx) / SLAB_DEAL_W] += work[t];
  std::vector<int> idx((size_t)gbx * gby);
  for (int g = 0; g < gbx * gby; ++g) idx[g] = g;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return gw[a] > gw[b]; });
  long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int g : idx) {
    int x = 0;
    for (int k = 1; k < 8; ++k)
      if (load[k] < load[x]) x = k;
    const int gy = g / gbx, gx = g - gy * gbx;
    for (int dy = 0; dy < SLAB_DEAL_H; ++dy)
      for (int dx = 0; dx < SLAB_DEAL_W; ++dx) {
        const int ty = gy * SLAB_DEAL_H + dy, tx = gx * SLAB_DEAL_W + dx;
        if (ty < P.nty && tx < P.ntx) run[x].push_back(ty * P.ntx + tx);
      }
    load[x] += gw[g];
  }
  // (a split tile's pieces weigh a share each: they sort behind the unsplit tiles of their tile's full weight)
  for (int x = 0; x < 8; ++x)
    std::stable_sort(run[x].begin(), run[x].end(), [&](int a, int b) { return work[a] / ksplit[a] > work[b] / ksplit[b]; });
  // a run's tiles become its workgroups {tile | piece << 20 | pieces << 26, cuts}, longest first by their own weights
  size_t longest = 0;
  std::vector<std::vector<std::pair<int, int2>>> items(8);
  for (int x = 0; x < 8; ++x) {
    for (int t : run[x]) {
      const unsigned char *c = &aux->cuts[(size_t)t * 10];
      for (int k = 0; k < c[0]; ++k)
        items[x].push_back({piece_weight(t, k), make_int2(t | (k << 20) | ((int)c[0] << 26), (int)c[1 + k] | ((int)c[2 + k] << 8))});
    }
    std::stable_sort(items[x].begin(), items[x].end(), [](const std::pair<int, int2> &a, const std::pair<int, int2> &b) { return a.first > b.first; });
    longest = std::max(longest, items[x].size());
  }
  order.assign(longest * 8, make_int2(-1, 0));
  for (int x = 0; x < 8; ++x)
    for (size_t k = 0; k < items[x].size(); ++k) order[k * 8 + x] = items[x][k].second;
  // ... followed by the list of split tiles for the merge pass (tile | pieces << 20), and their number last
  int nsplit = 0;
  for (int t = 0; t < nt; ++t)
    if (ksplit[t] > 1) { order.push_back(make_int2(t | ((int)ksplit[t] << 20), 0)); ++nsplit; }
  order.push_back(make_int2(nsplit, 0));
  aux->plan_work = work;
  aux->plan_cuts = aux->cuts;
  aux->plan_order = order;
  aux->plan_slots = slots;
}

// the split tiles of the schedule: pieces per tile (stat "slab_split_tiles"), and room for their partial frames.
// *nblocks = workgroups of the kernel.
static hipError_t slab_segments(const RenderParams &P, SlabParams &Q, SlabAux *aux, const std::vector<int2> &order, int *nblocks) {
  const int nt = P.ntx * P.nty;
  const int nsplit = order.back().x;
  *nblocks = (int)order.size() - 1 - nsplit;
  aux->ksplit_last.assign((size_t)nt, 1);
  int maxseg = 1;
  for (int k = 0; k < nsplit; ++k) {
    const int code = order[(size_t)*nblocks + k].x;
    aux->ksplit_last[code & 0xfffff] = (unsigned char)(code >> 20);
    maxseg = std::max(maxseg, code >> 20);
  }
  aux->nsplit_last = nsplit;
  aux->nblocks_last = *nblocks;
  if (maxseg > 1) {
    // (room for the largest piece count at once: growing the buffer when a tile's count rises is a hipFree + hipMalloc,
    //  ~1 ms in the middle of a session -- 7 partial frames of a 1024^2 viewport are 112 MB of 288 GB)
    const size_t need = (size_t)(8 - 1) * P.W * P.H * 16;
    if (need > aux->seg_cap) {
      if (aux->d_seg) (void)hipFree(aux->d_seg);
      aux->d_seg = nullptr;
      aux->seg_cap = 0;
      hipError_t e = hipMalloc(&aux->d_seg, need);
      if (e != hipSuccess) return e;
      aux->seg_cap = need;
    }
  }
  Q.seg_out = (float4 *)aux->d_seg;
  return hipSuccess;
}

// ---- order upload: the schedule to aux->d_order, when it changed
static hipError_t slab_upload_order(SlabAux *aux, std::vector<int2> &order, hipStream_t s) {
  if (aux->frame_ev0) {  // the frame's kernel-time bracket opens here: planning is done
    hipError_t e = hipEventRecord(aux->frame_ev0, s);
    if (e != hipSuccess) return e;
  }
  auto same_order = [&]() { return aux->order_host.size() == order.size() && (order.empty() || !memcmp(aux->order_host.data(), order.data(), order.size() * sizeof(int2))); };
  if (!same_order()) {  // unchanged camera: the table on the device is still right
    if ((int)order.size() > aux->order_cap) {
      if (aux->d_order) (void)hipFree(aux->d_order);
      aux->d_order = nullptr;
      for (int k = 0; k < 4; ++k) {
        if (aux->order_ev[k]) (void)hipEventSynchronize(aux->order_ev[k]);
        if (aux->h_order[k]) (void)hipHostFree(aux->h_order[k]);
        aux->h_order[k] = nullptr;
      }
      aux->order_cap = 0;
      // (with headroom: the table grows by a few entries whenever a tile's piece count rises, and every regrowth is a
      //  device free + allocation and four pinned ones -- a 1 ms hiccup every few dozen frames on a shard)
      const size_t cap = order.size() * 2 + 1024;
      hipError_t e = hipMalloc((void **)&aux->d_order, cap * sizeof(int2));
      for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipHostMalloc((void **)&aux->h_order[k], cap * sizeof(int2), hipHostMallocDefault);
      if (e != hipSuccess) return e;
      aux->order_cap = (int)cap;
    }
    // pinned staging + a copy ON THE LAUNCH STREAM: a copy from pageable memory is not
    // stream-ordered against the kernel that follows (seen as wrong tiles when several
    // contexts render at once).  Four staging buffers in turn, each rewritten only after its
    // own last copy: the host does not wait for the stream unless it is four tables ahead.
    const int k = aux->order_next;
    aux->order_next = (k + 1) & 3;
    hipError_t e = aux->order_ev[k] ? hipEventSynchronize(aux->order_ev[k]) : hipEventCreateWithFlags(&aux->order_ev[k], hipEventDisableTiming);
    if (e != hipSuccess) return e;
    memcpy(aux->h_order[k], order.data(), order.size() * sizeof(int2));
    e = hipMemcpyAsync(aux->d_order, aux->h_order[k], order.size() * sizeof(int2), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    e = hipEventRecord(aux->order_ev[k], s);
    if (e != hipSuccess) return e;
    aux->order_host.swap(order);
  }
  return hipSuccess;
}

// per-workgroup timeline records (option lockstep bit 32)
static hipError_t slab_trace(const RenderParams &P, SlabParams &Q, SlabAux *aux, int nblocks, hipStream_t s) {
  Q.trace = nullptr;
  if (!(P.lockstep & 32)) return hipSuccess;
  if (nblocks > aux->trace_cap) {
    if (aux->d_trace) (void)hipFree(aux->d_trace);
    aux->d_trace = nullptr;
    aux->trace_cap = 0;
    hipError_t e = hipMalloc((void **)&aux->d_trace, (size_t)nblocks * 32);
    if (e != hipSuccess) return e;
    aux->trace_cap = nblocks;
  }
  hipError_t e = hipMemsetAsync(aux->d_trace, 0, (size_t)nblocks * 32, s);
  if (e != hipSuccess) return e;
  aux->trace_n = nblocks;
  Q.trace = aux->d_trace;
  return hipSuccess;
}

// ---- launch: the merge pass's warm-up, the kernel, the merge pass, and the read-back of the tick words (the next
// frames' weights)
static hipError_t slab_run(const RenderParams &P, const SlabParams &Q, SlabAux *aux, int dtype, int tf_mode, int shade_kind, SlabShape sh,
                           size_t lds, int nblocks, long long tsig, const char **why, hipStream_t s) {
  const int nt = Q.ntiles, nsplit = aux->nsplit_last;
  hipError_t e = nsplit > 0 ? hipMemsetAsync(aux->d_ticks, 0, (size_t)nt * 20, s) : hipSuccess;  // (their tick words are sums over the pieces)
  if (e != hipSuccess) return e;
  // (the merge pass's first launch costs the host a few milliseconds of code loading, which lands between the frame's
  //  events: paid here, in a context's first slice-ring frame -- not in the frame auto mode happens to be timing when
  //  the first tiles are cut.  One block whose entry names tile 0 with ONE piece: it rewrites that tile's pixels with
  //  themselves, before this frame's kernel writes them.)
  if (!aux->merge_warm && nblocks >= 1) {
    aux->merge_warm = true;
    static const int2 one = make_int2(0 | (1 << 20), 0);
    int2 *d_one = nullptr;
    if (hipMalloc((void **)&d_one, sizeof one) == hipSuccess) {
      if (hipMemcpyAsync(d_one, &one, sizeof one, hipMemcpyHostToDevice, s) == hipSuccess)
        (void)smk_slab_merge(d_one, 1, sh.tw, sh.th, P.ntx, P.W, P.H, (const float4 *)P.out, P.out, 0, s);
      (void)hipStreamSynchronize(s);
      (void)hipFree(d_one);
    }
    (void)hipGetLastError();
  }
  e = smk_slab_launch_instance(slab_inst_for(P, Q, dtype, tf_mode, shade_kind, sh), P, Q, lds, nblocks, why, s);
  if (e == hipSuccess && nsplit > 0)
    e = smk_slab_merge(aux->d_order + nblocks, nsplit, sh.tw, sh.th, P.ntx, P.W, P.H, (const float4 *)aux->d_seg, P.out,
                       P.blend == SMK_BLEND_MAX ? 1 : 0, s);
  if (e != hipSuccess || aux->ticks_pending) return e;
  // fetch this frame's per-tile durations (one copy in flight at a time)
  e = hipMemcpyAsync(aux->h_ticks, aux->d_ticks, (size_t)nt * 4, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && nsplit > 0) e = hipMemcpyAsync(aux->h_pticks, aux->d_pticks, (size_t)nt * 32, hipMemcpyDeviceToHost, s);
  if (nsplit > 0) aux->cuts_pending = aux->cuts; else aux->cuts_pending.clear();
  if (e == hipSuccess) e = hipEventRecord(aux->ticks_ev, s);
  if (e != hipSuccess) return e;
  aux->ticks_pending = true;
  aux->ticks_pending_sig = tsig;
  aux->ticks_pending_n = nt;
  return hipSuccess;
}

// ---- the plan of the latest launch, for smk_get_stat "slab_plan_<field>" (include/smk.h): host memory only, no
// synchronisation; 0 unless the latest frame ran the slice-ring kernel
static const char *const SLAB_PLAN_NAMES[SlabAux::PLAN_FIELDS] = {
    "tw", "th", "nw", "nl", "wu", "wv", "wp", "per", "rpg", "groups", "chunks", "mych", "nslots", "maxfly", "wstep", "pmask", "mask_need",
    "use_occ", "use_ah", "fast_tf", "bricks", "perm", "dir", "lds_bytes", "slices_max"};
static void slab_keep_plan(const SlabParams &Q, SlabShape sh, size_t lds, SlabAux *aux) {
  const int nw = slab_waves(sh), nlg = slab_loader_groups(nw, sh.nl), lpg = sh.nl / nlg;
  const int mych = (Q.groups + lpg - 1) / lpg * Q.per;  // (slab_ring's)
  const int v[SlabAux::PLAN_FIELDS] = {sh.tw, sh.th, nw, sh.nl, Q.wu, Q.wv, Q.wp, Q.per, Q.rpg, Q.groups, Q.chunks, mych, Q.nslots, Q.maxfly,
                                       Q.wstep, Q.pmask, Q.mask_need, Q.use_occ, Q.use_ah, Q.fast_tf, Q.bricks ? 1 : 0, Q.perm, Q.dir, (int)lds,
                                       aux->scan_slices};
  memcpy(aux->plan_last, v, sizeof v);
}
int smk_slab_plan_stat(smk_ctx *c, const char *name, double *value) {
  for (int k = 0; k < SlabAux::PLAN_FIELDS; ++k)
    if (!strcmp(name + 10, SLAB_PLAN_NAMES[k])) {
      *value = c->last_kernel == 2 ? c->slab.plan_last[k] : 0;
      return 0;
    }
  FAIL(c, "smk_get_stat: unknown name '%s'", name);
}

static hipError_t slab_plan_and_launch(RenderParams &P, int dtype, int tf_mode, int shade_kind, const void *vox_native, const void *vox_xmajor,
                                       SlabAux *aux, const char **why, hipStream_t s) {
  const double t0 = slab_clock.on ? slab_now() : 0;
  slab_clock.frame_scan = 0;
  SlabParams Q;
  memset(&Q, 0, sizeof Q);
  Q.status = aux->h_status + aux->status_slot;
  Q.status_tag = aux->status_tag;
  Q.diag = aux->d_diag;
  const double ds = slab_axes(P, vox_native, vox_xmajor, Q);
  if ((*why = slab_refusal(P, dtype, tf_mode, Q))) return hipErrorNotSupported;
  if (tf_mode == 0) shade_kind = 0;  // (the scalar renderer does not shade, VolumeRenderer.cpp:576-587)
  SlabShape shape;
  size_t lds = 0;
  std::vector<int> work;
  if ((*why = slab_choose_shape(P, Q, dtype, tf_mode, shade_kind, ds, aux, shape, &lds, work))) return hipErrorNotSupported;

  const int nw = slab_waves(shape), nt = P.ntx * P.nty;
  const long long tsig = (((long long)P.ntx * 4096 + P.nty) * 64 + shape.tw) * 64 + shape.th + ((long long)(Q.perm * 2 + (Q.dir > 0)) << 48) +
                         ((long long)nw << 52) + ((long long)dtype << 56);
  hipError_t e = slab_measured_weights(aux, tsig, nt, work, Q);
  if (e != hipSuccess) return e;
  // DEPTH SEGMENTS: 0 auto (measured long tiles), 1 off, 2.. every tile in that many (a depth output: off -- the merge
  // pass knows colours only)
  const int opt_split = P.depth ? 1 : aux->opt_split;
  slab_cut_segments(aux, work, nt, tsig, opt_split, slab_big(nw, shape.nl));
  std::vector<int2> order;
  slab_schedule(P, aux, work, (nw + shape.nl) | (opt_split << 12), order);
  int nblocks = 0;
  if ((e = slab_segments(P, Q, aux, order, &nblocks)) != hipSuccess) return e;
  if (slab_clock.on) {
    slab_clock.scan += slab_clock.frame_scan;
    slab_clock.planned += slab_now() - t0;
    if (++slab_clock.n % 60 == 0) {
      fprintf(stderr, "[smk] planning per frame: scans %.3f ms, all of it up to the launch %.3f ms, whole launcher (previous 60) %.3f ms\n",
              slab_clock.scan / 60, slab_clock.planned / 60, slab_clock.whole / 60);
      slab_clock.scan = slab_clock.planned = slab_clock.whole = 0;
    }
  }
  if ((e = slab_upload_order(aux, order, s)) != hipSuccess) return e;
  Q.order = aux->d_order;
  if ((e = slab_trace(P, Q, aux, nblocks, s)) != hipSuccess) return e;
  slab_keep_plan(Q, shape, lds, aux);
  return slab_run(P, Q, aux, dtype, tf_mode, shade_kind, shape, lds, nblocks, tsig, why, s);
}

hipError_t smk_launch_slab(RenderParams P, int dtype, int tf_mode, int shade_kind, const void *vox_native, const void *vox_xmajor, SlabAux *aux,
                           const char **why, hipStream_t s) {
  const double t0 = slab_clock.on ? slab_now() : 0;
  const hipError_t e = slab_plan_and_launch(P, dtype, tf_mode, shade_kind, vox_native, vox_xmajor, aux, why, s);
  if (slab_clock.on) slab_clock.whole += slab_now() - t0;
  return e;
}
