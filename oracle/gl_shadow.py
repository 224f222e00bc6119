"""An independent witness for the half-angle-slicing shadow mode: the GL slice pipeline of R8kVolRen3D in float64.

TEST INFRASTRUCTURE ONLY (imported by tests/ alone).  oracle/smk_oracle.c (orc_shadow_setup / orc_render_shadow) places
its eye samples with the product's own fma chain (smk_ray_AB) and its light samples with the product's light rays, so a
misreading shared by the two would pass every parity test.  This module derives the same frame the way the pipeline drew
it -- slice polygons, two rasterisations per slice, texture fetches, the shader's arithmetic, the framebuffer blend -- with
nothing taken from the checker's coefficients:

  * half vector and order (R8kVolRen3D.cpp:296-320): v = the view direction, l = -norm(light.pos); v negated when
    v.l <= 0; h = (v - l)/2 + l, taken to model space by xform's inverse (mvinv . axis, :1321-1324); front to back
    (GL_ONE_MINUS_DST_ALPHA, GL_ONE) when v.l > 0, else back to front (GL_ONE, GL_ONE_MINUS_SRC_ALPHA) (:1436-1449);
  * slice planes (:1321-1351, with the plane-set convention the project documents in DESIGN.md section 8): sn.X = tmin +
    k dc, k = 1..S, tmin / tmax over the whole volume's corners; dc = the reference's dis = xfSize / (xiSize * rate)
    (float, :1330) and S = (int)((tmax - tmin) / dc) in float64, or, in steps mode, dc = (tmax - tmin) / steps;
  * slice polygons: each plane cut against the 12 edges of the box (`intersect`, as oracle/gl_slices.py), the box being
    the volume or what an orthogonal clip plane leaves of it; a free clip plane is a per-fragment half-space test;
  * eye pass of slice k: the polygon through modelview, glFrustum and the viewport, rasterised at pixel centres as a
    triangle fan with perspective-correct model coordinates; per fragment a GL_LINEAR clamp-to-edge fetch of the volume
    and its normals, the 2-D (x optional H) or dense 3-D table, shading off or the R8k form, the light buffer as slices
    1..k-1 left it looked up through ltxf = light.xf . xform . tb (:1280-1290; light.xf = LTWidgetRen::genXForm,
    LTWidgetRen.cpp:231-291) at lc = (x'/w . .85 + .5) . quality (:1673-1674), bilinear, border 0; colour times
    1 - light.rgb (:2928-2934), then the blend;
  * light pass of slice k: the same polygon rasterised under ltxf into the LB x LB buffer (LB = ceil(quality buffer_px)),
    L.rgb = sat(lerp(L.rgb, colour, a)), L.a = sat((1 - a) L.a + a) (:3150-3165).

Ambiguity: the only discontinuities of the frame are the box faces and the clip planes (every table is bilinear).  A
sample within DELTA voxels outside (INSIDE inside) of one of them is flagged; a pixel is ambiguous when one of its samples is flagged or reads a
flagged light texel; a texel is ambiguous from the first slice that flagged it on.  A slice plane that lies ON a box face
(the last slice of steps mode with an axis-aligned half vector) is drawn: GL rasterises that polygon, so it is not
ambiguous.
"""
import numpy as np

# Ambiguity band around a box face, in voxels: a sample up to DELTA outside or INSIDE inside a face is flagged.  Outside:
# the product and the checker take every sample within 2^-10 voxels of the box (SMK_SHADOW_BOX_EPS), which GL would not
# draw, plus their fp32 placement error (< 5e-5 voxels, tests/test_shadow_witness.py::test_placement_...).  Inside: the
# placement error alone.  Clip planes: DELTA on both sides.
DELTA = 2e-3
INSIDE = 1e-4

# box vertices x fastest (bit 0 = x, 1 = y, 2 = z) and the 12 edges of render3DVA's intersect() calls (:1473-1507)
EDGES = [(0, 1), (0, 2), (1, 3), (4, 0), (1, 5), (2, 3), (4, 5), (4, 6), (5, 7), (6, 7), (2, 6), (3, 7)]


def _normalise(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def look_at(eye, at, up):
    """gluLookAt as a 4x4 matrix (row-major maths convention)"""
    eye = np.asarray(eye, np.float64)
    F = _normalise(np.asarray(at, np.float64) - eye)
    s = _normalise(np.cross(F, np.asarray(up, np.float64)))
    u = np.cross(s, F)
    M = np.eye(4)
    M[0, :3], M[1, :3], M[2, :3] = s, u, -F
    T = np.eye(4)
    T[:3, 3] = -eye
    return M @ T


def translate(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def frustum(l, r, b, t, n, f):
    return np.array([[2 * n / (r - l), 0, (r + l) / (r - l), 0],
                     [0, 2 * n / (t - b), (t + b) / (t - b), 0],
                     [0, 0, -(f + n) / (f - n), -2 * f * n / (f - n)],
                     [0, 0, -1, 0]], np.float64)


def light_xf(light_pos):
    """LTWidgetRen::genXForm: pj . mv with mv = gluLookAt(-norm(light.pos), 0, y) whose z translation is negated, pj the
    identity with pj[11] = 1/d0 (column-major: row 3, column 2)"""
    d0 = np.linalg.norm(np.asarray(light_pos, np.float64))
    mv = look_at(-_normalise(light_pos), (0, 0, 0), (0, 1, 0))
    mv[2, 3] = -mv[2, 3]
    pj = np.eye(4)
    pj[3, 2] = 1.0 / d0
    return pj @ mv


def _solve_on_plane(M, win_to_ndc, xs, ys, sn, c):
    """model points on the plane sn.X = c whose projection under M (rows 0, 1, 3 used: x/w, y/w) is the window point
    (xs, ys): a 3x3 solve per point (the direct ray-plane intersection)"""
    nx = (xs - win_to_ndc[0][1]) / win_to_ndc[0][0]
    ny = (ys - win_to_ndc[1][1]) / win_to_ndc[1][0]
    shp = nx.shape
    nx, ny = nx.reshape(-1), ny.reshape(-1)
    A = np.empty((nx.size, 3, 3))
    rhs = np.empty((nx.size, 3))
    A[:, 0] = M[0, :3][None] - nx[:, None] * M[3, :3][None]
    rhs[:, 0] = nx * M[3, 3] - M[0, 3]
    A[:, 1] = M[1, :3][None] - ny[:, None] * M[3, :3][None]
    rhs[:, 1] = ny * M[3, 3] - M[1, 3]
    A[:, 2] = sn[None]
    rhs[:, 2] = c
    X = np.linalg.solve(A, rhs[..., None])[..., 0]
    return X.reshape(shp + (3,))


def _raster(M, win_to_ndc, poly, W, H):
    """rasterise the convex model-space polygon under M at pixel centres of a W x H target: triangle fan, perspective-
    correct interpolation of the model coordinates.  Returns (covered [H][W], X [H][W][3])"""
    clip = (M @ np.concatenate([poly, np.ones((len(poly), 1))], axis=1).T).T
    w = clip[:, 3]
    win = np.stack([clip[:, 0] / w * win_to_ndc[0][0] + win_to_ndc[0][1],
                    clip[:, 1] / w * win_to_ndc[1][0] + win_to_ndc[1][1]], axis=1)
    cen = win.mean(axis=0)
    order = np.argsort(np.arctan2(win[:, 1] - cen[1], win[:, 0] - cen[0]))
    win, w, poly = win[order], w[order], poly[order]
    px = (np.arange(W) + 0.5)[None, :]
    py = (np.arange(H) + 0.5)[:, None]
    # coverage by the polygon's own edges (counter-clockwise after the sort): the fan's inner diagonals are no boundary,
    # so a pixel centre on one is covered once, as GL's watertight rule has it
    covered = np.ones((H, W), bool)
    for j in range(len(win)):
        a, b = win[j], win[(j + 1) % len(win)]
        covered &= (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0]) >= 0
    # interpolation: the fan triangle the centre lies deepest in, perspective-correct
    best = np.full((H, W), -np.inf)
    X = np.zeros((H, W, 3))
    for k in range(1, len(win) - 1):
        a, b, c = win[0], win[k], win[k + 1]
        den = (b[1] - c[1]) * (a[0] - c[0]) + (c[0] - b[0]) * (a[1] - c[1])
        if abs(den) < 1e-12:
            continue
        l0 = ((b[1] - c[1]) * (px - c[0]) + (c[0] - b[0]) * (py - c[1])) / den
        l1 = ((c[1] - a[1]) * (px - c[0]) + (a[0] - c[0]) * (py - c[1])) / den
        l2 = 1 - l0 - l1
        depth = np.minimum(np.minimum(l0, l1), l2)
        take = depth > best
        i0, i1, i2 = l0 / w[0], l1 / w[k], l2 / w[k + 1]
        q = i0 + i1 + i2
        Xk = (i0[..., None] * poly[0] + i1[..., None] * poly[k] + i2[..., None] * poly[k + 1]) / q[..., None]
        X[take] = Xk[take]
        best = np.maximum(best, depth)
    return covered, X


def _linear_axis(u, n):
    """GL_LINEAR clamp-to-edge along one axis, u in texel units (coordinate * n - 0.5)"""
    u = np.clip(u, 0.0, n - 1.0)
    i0 = np.minimum(np.floor(u).astype(np.int64), max(n - 2, 0))
    return i0, np.minimum(i0 + 1, n - 1), u - i0


def _tex3(vol, p):
    """trilinear fetch of vol [z][y][x][C] at voxel coordinates p [..., 3] (x, y, z)"""
    nz, ny, nx = vol.shape[:3]
    x0, x1, fx = _linear_axis(p[..., 0], nx)
    y0, y1, fy = _linear_axis(p[..., 1], ny)
    z0, z1, fz = _linear_axis(p[..., 2], nz)
    out = 0.0
    for zi, wz in ((z0, 1 - fz), (z1, fz)):
        for yi, wy in ((y0, 1 - fy), (y1, fy)):
            for xi, wx in ((x0, 1 - fx), (x1, fx)):
                out = out + (wz * wy * wx)[..., None] * vol[zi, yi, xi]
    return out


def _tex2(tab, s, t):
    """GL_LINEAR clamp-to-edge lookup of an RGBA8 table tab [t][s][4] at s, t in [0, 1] -> [..., 4] in [0, 1]"""
    st, ss = tab.shape[:2]
    s0, s1, fs = _linear_axis(s * ss - 0.5, ss)
    t0, t1, ft = _linear_axis(t * st - 0.5, st)
    T = tab.astype(np.float64) / 255.0
    a = (1 - fs)[..., None] * T[t0, s0] + fs[..., None] * T[t0, s1]
    b = (1 - fs)[..., None] * T[t1, s0] + fs[..., None] * T[t1, s1]
    return (1 - ft)[..., None] * a + ft[..., None] * b


def _tex3tab(tab, s, t, r):
    """dense 3-D table tab [r][t][s][4] (r = H, t = G, s = V), GL_LINEAR clamp-to-edge"""
    sr, st, ss = tab.shape[:3]
    p = np.stack([s * ss - 0.5, t * st - 0.5, r * sr - 0.5], axis=-1)
    return _tex3(tab.astype(np.float64) / 255.0, p)


def _bilinear_border0(L, lx, ly):
    """GL_LINEAR, GL_CLAMP with a zero border: L [LB][LB][C] at texel coordinates (lx, ly).  Also the four taps."""
    LB = L.shape[0]
    fx0, fy0 = np.floor(lx - 0.5), np.floor(ly - 0.5)
    fx, fy = lx - 0.5 - fx0, ly - 0.5 - fy0
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    out = 0.0
    taps = []
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            x, y = x0 + dx, y0 + dy
            ok = (x >= 0) & (x < LB) & (y >= 0) & (y < LB)
            v = np.where(ok[..., None], L[np.clip(y, 0, LB - 1), np.clip(x, 0, LB - 1)], 0.0)
            out = out + (wx * wy)[..., None] * v
            taps.append((np.clip(x, 0, LB - 1), np.clip(y, 0, LB - 1), ok))
    return out, taps


class _Setup:
    """everything of one frame that does not depend on the slice"""

    def __init__(self, sc, delta):
        self.sc = sc
        self.delta = delta
        self.N = np.array(sc.dims, np.float64)
        self.f = np.array([float(v) for v in sc.fsize], np.float64)
        self.xf = np.array(sc.xform, np.float64).reshape(4, 4).T
        self.MV = look_at(sc.eye, sc.at, sc.up) @ translate(*sc.trans) @ self.xf @ translate(*(-self.f / 2))
        l, r, b, t = (float(v) for v in sc.frustum)
        self.PM = frustum(l, r, b, t, float(sc.znear), 20.0) @ self.MV
        self.W, self.H = sc.width, sc.height
        self.eye_win = ((0.5 * self.W, 0.5 * self.W), (0.5 * self.H, 0.5 * self.H))
        # half vector and blend order (:296-320, :1436-1449)
        vd = _normalise(np.asarray(sc.at, np.float64) - np.asarray(sc.eye, np.float64))
        ld = -_normalise(sc.light_pos)
        vdl = float(vd @ ld)
        self.front_to_back = vdl > 0
        if vdl <= 0:
            vd = -vd
        h = (vd - ld) * 0.5 + ld
        sn = np.linalg.inv(self.xf[:3, :3]) @ h
        self.sn = sn / np.linalg.norm(sn)
        # plane set over the whole volume (:1321-1351)
        corners = np.array([[(i & 1) * self.f[0], ((i >> 1) & 1) * self.f[1], ((i >> 2) & 1) * self.f[2]] for i in range(8)])
        tt = corners @ self.sn
        self.tmin, self.tmax = float(tt.min()), float(tt.max())
        if sc.steps > 0:
            self.S = int(sc.steps)
            self.dc = (self.tmax - self.tmin) / self.S
        else:
            self.dc = float(np.float32(self.f[0]) / (np.float32(sc.dims[0]) * np.float32(sc.sample_rate)))
            self.S = int((self.tmax - self.tmin) / self.dc)
        # the sliced box, model space: the volume or what the orthogonal clip plane leaves of it
        lo, hi = np.zeros(3), self.f.copy()
        if sc.clip and 1 <= sc.clip[0] <= 6:
            a = (sc.clip[0] - 1) // 2
            cp = min(max(float(sc.clip[1][a]), 0.0), self.f[a])
            if (sc.clip[0] - 1) % 2 == 0:
                hi[a] = min(hi[a], cp)
            else:
                lo[a] = max(lo[a], cp)
        self.blo, self.bhi = lo, hi
        self.box = np.array([[hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]] for i in range(8)])
        self.vlo, self.vhi = self.to_voxel(lo), self.to_voxel(hi)
        # a face the slice planes are parallel to: a plane ON it is the face itself (drawn), not its edge
        self.parallel = np.abs(self.sn) > 1.0 - 1e-12
        # free clip plane, model space: keep pm . (X, 1) >= 0
        self.pm = None
        if sc.clip_plane is not None:
            self.pm = self.MV.T @ np.asarray(sc.clip_plane, np.float64)
            self.pm_vox_norm = np.linalg.norm(self.pm[:3] * self.f / self.N)
        # light: ltxf = light.xf . xform . tb (:1280-1290), tb = translate(-fSize/2) for the whole volume
        self.LT = light_xf(sc.light_pos) @ self.xf @ translate(*(-self.f / 2))
        LBf = float(sc.shadow[1]) * float(sc.shadow[0])
        self.LBf = LBf
        self.LB = int(np.ceil(LBf))
        self.light_win = ((0.85 * LBf, 0.5 * LBf), (0.85 * LBf, 0.5 * LBf))
        # shading (R8kVolRen3D.cpp:2625-2640): L = -norm(light.pos), H = norm(L + (V - L)/2), V = norm(at - eye)
        self.Ls = -_normalise(sc.light_pos)
        V = _normalise(np.asarray(sc.at, np.float64) - np.asarray(sc.eye, np.float64))
        self.Hs = _normalise(self.Ls + 0.5 * (V - self.Ls))
        d = sc.data
        self.vol = d.astype(np.float64) / 255.0 if d.dtype == np.uint8 else d.astype(np.float64)
        if self.vol.shape[3] < 4:
            self.vol = np.concatenate([self.vol, np.zeros(self.vol.shape[:3] + (4 - self.vol.shape[3],))], axis=3)
        self.grad = sc.grad.astype(np.float64) if sc.grad is not None else None

    def to_voxel(self, X):
        return X / self.f * self.N - 0.5

    def plane(self, k):
        return self.tmin + k * self.dc

    def polygon(self, c):
        pts = []
        for a, b in EDGES:
            p0, p1 = self.box[a], self.box[b]
            den = self.sn @ (p1 - p0)
            if abs(den) < 1e-12:
                continue
            t = (c - self.sn @ p0) / den
            if -1e-9 <= t <= 1 + 1e-9:
                pts.append(p0 + min(max(t, 0.0), 1.0) * (p1 - p0))
        if len(pts) < 3:
            return None
        pts = np.unique(np.round(np.array(pts), 12), axis=0)
        return pts if len(pts) >= 3 else None

    def flags(self, X):
        """samples within delta voxels of a box face (not one the plane lies on) or of the free clip plane"""
        p = self.to_voxel(X)
        d = self.delta
        di = INSIDE
        grown = np.all((p >= self.vlo - d) & (p <= self.vhi + d), axis=-1)
        near = (((p - self.vlo > -d) & (p - self.vlo < di)) | ((self.vhi - p > -d) & (self.vhi - p < di))) & ~self.parallel
        f = grown & near.any(axis=-1)
        if self.pm is not None:
            f |= grown & (np.abs(X @ self.pm[:3] + self.pm[3]) < d * self.pm_vox_norm)
        return f

    def kept(self, X):
        if self.pm is None:
            return np.ones(X.shape[:-1], bool)
        return X @ self.pm[:3] + self.pm[3] >= 0

    def classify(self, ch):
        sc = self.sc
        if sc.tf_mode == 1:
            col = _tex2(sc.tf_vg, ch[..., 0], ch[..., 1])
            if sc.third_axis and sc.tf_h is not None:
                col[..., 3] = col[..., 3] * _tex2(sc.tf_h, ch[..., 2], ch[..., 3])[..., 3]
        elif sc.tf_mode == 2:
            col = _tex3tab(sc.tf3d, ch[..., 0], ch[..., 1], ch[..., 2])
        else:
            raise ValueError("shadows take a 2-D or 3-D transfer function")
        col[..., 3] = np.clip(col[..., 3], 0.0, 1.0)
        return col

    def light_project(self, X):
        q = X @ self.LT[:3, :3].T + self.LT[:3, 3]
        w = X @ self.LT[3, :3] + self.LT[3, 3]
        return ((q[..., 0] / w) * 0.85 + 0.5) * self.LBf, ((q[..., 1] / w) * 0.85 + 0.5) * self.LBf

    def shade(self, p, ch, col, shadow):
        """the eye pass's fragment: premultiplied src (R8kVolRen3D.cpp:2831-2846, 2886-2934, 2974-2977)"""
        sc = self.sc
        a = col[..., 3]
        c = col[..., :3].copy()
        if sc.shade_mode == 1 and self.grad is not None:
            n = _tex3(self.grad, p) * (2.0 / 255.0) - 1.0
            w = n @ self.xf[:3, :3].T                       # the normal taken to world space
            ln = np.linalg.norm(w, axis=-1, keepdims=True)
            w = np.where(ln > 0, w / np.where(ln > 0, ln, 1.0), 0.0)
            kd = np.clip(np.maximum(np.clip(np.abs(w @ self.Ls), 0, 1), 0.2), 0, 1) * sc.intens
            ks = np.clip(np.clip(np.abs(w @ self.Hs), 0, 1) ** 30, 0, 1) * sc.intens if sc.use_spec else 0.0 * kd
            shaded = c * kd[..., None] + ks[..., None]
            c = c + ch[..., 1:2] * (shaded - c)              # LERP by the second data channel
        elif sc.shade_mode not in (0, 1):
            raise ValueError("shadows take shading off or the R8k form")
        c = c * (1.0 - shadow)                               # MUL r0, r0, 1 - r5
        return np.concatenate([np.clip(c * a[..., None], 0, 1), a[..., None]], axis=-1)


def render_shadow(sc, delta=DELTA):
    """the half-angle-slicing frame of oracle.Scene `sc` (sc.shadow = (buffer_px, quality)).  Returns a dict:
      rgba [H][W][4] premultiplied, row 0 = bottom;  light [LB][LB][4] the final light buffer;
      history [S+1][LB][LB][4] the buffer after slices 1..k (history[0] = cleared);  depth [H][W] view depth of the
      nearest sample with alpha > 0 (+inf where none);  amb [H][W] ambiguous pixels;  lamb [LB][LB] ambiguous texels
      after the last slice; lamb_history [S+1][LB][LB];  bound [H][W] / lbound [LB][LB] the largest single-slice
      contribution (alpha) to each pixel / texel;  front_to_back, nslices, sn, planes (tmin, dc)."""
    g = _Setup(sc, delta)
    W, H, LB, S = g.W, g.H, g.LB, g.S
    C = np.zeros((H, W, 4))
    depth = np.full((H, W), np.inf)
    amb = np.zeros((H, W), bool)
    bound = np.zeros((H, W))
    L = np.zeros((LB, LB, 4))
    lamb = np.zeros((LB, LB), bool)
    lbound = np.zeros((LB, LB))
    hist = np.zeros((S + 1, LB, LB, 4))
    lamb_hist = np.zeros((S + 1, LB, LB), bool)
    pxc, pyc = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    txc, tyc = np.meshgrid(np.arange(LB) + 0.5, np.arange(LB) + 0.5)
    for k in range(1, S + 1):
        c = g.plane(k)
        poly = g.polygon(c)
        # ---- eye pass: reads L as slices 1..k-1 left it
        Xd = _solve_on_plane(g.PM, g.eye_win, pxc, pyc, g.sn, c)
        fl = g.flags(Xd)
        if fl.any():            # (a flagged sample the other side may draw: its alpha bounds what it can change)
            amb |= fl
            bound[fl] = np.maximum(bound[fl], g.classify(_tex3(g.vol, g.to_voxel(Xd[fl])))[:, 3])
        if poly is not None:
            cov, X = _raster(g.PM, g.eye_win, poly, W, H)
            cov &= g.kept(X)
            if cov.any():
                Xs = X[cov]
                p = g.to_voxel(Xs)
                ch = _tex3(g.vol, p)
                col = g.classify(ch)
                lx, ly = g.light_project(Xs)
                shadow, taps = _bilinear_border0(L[..., :3], lx, ly)
                src = g.shade(p, ch, col, shadow)
                a = src[..., 3]
                live = a > 0
                rd = np.zeros(len(Xs), bool)
                for tx, ty, ok in taps:
                    rd |= ok & lamb[ty, tx]
                idx = np.nonzero(cov)
                amb[idx[0][rd & live], idx[1][rd & live]] = True
                bound[idx] = np.maximum(bound[idx], a)
                Cp = C[idx]
                if g.front_to_back:
                    Cp = Cp + (1 - Cp[:, 3:4]) * src
                else:
                    Cp = src + (1 - a[:, None]) * Cp
                C[idx] = np.where(live[:, None], Cp, C[idx])
                zeye = -(Xs @ g.MV[2, :3] + g.MV[2, 3])     # view depth of the sample
                dp = depth[idx]
                depth[idx] = np.where(live, np.minimum(dp, zeye), dp)
        # ---- light pass: slice k composited onto L
        Xl = _solve_on_plane(g.LT, g.light_win, txc, tyc, g.sn, c)
        fl = g.flags(Xl)
        if fl.any():
            lamb |= fl
            lbound[fl] = np.maximum(lbound[fl], g.classify(_tex3(g.vol, g.to_voxel(Xl[fl])))[:, 3])
        if poly is not None:
            cov, X = _raster(g.LT, g.light_win, poly, LB, LB)
            cov &= g.kept(X)
            if cov.any():
                Xs = X[cov]
                col = g.classify(_tex3(g.vol, g.to_voxel(Xs)))
                a = col[:, 3:4]
                Lo = L[cov]
                Ln = np.empty_like(Lo)
                Ln[:, :3] = np.clip(a * np.clip(col[:, :3], 0, 1) + (1 - a) * Lo[:, :3], 0, 1)
                Ln[:, 3] = np.clip((1 - a[:, 0]) * Lo[:, 3] + a[:, 0], 0, 1)
                L[cov] = Ln
                lbound[cov] = np.maximum(lbound[cov], a[:, 0])
        hist[k] = L
        lamb_hist[k] = lamb
    return dict(rgba=C, light=L, history=hist, depth=depth, amb=amb, lamb=lamb, lamb_history=lamb_hist, bound=bound,
                lbound=lbound, front_to_back=g.front_to_back, nslices=S, sn=g.sn, planes=(g.tmin, g.dc), setup=g)


def eye_samples(sc, k, delta=DELTA):
    """slice k's plane point of every pixel's ray in voxel coordinates [H][W][3] (the direct ray-plane intersection)"""
    g = _Setup(sc, delta)
    pxc, pyc = np.meshgrid(np.arange(g.W) + 0.5, np.arange(g.H) + 0.5)
    return g.to_voxel(_solve_on_plane(g.PM, g.eye_win, pxc, pyc, g.sn, g.plane(k))), g
