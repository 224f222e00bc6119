"""The float64 half-angle slice pipeline of oracle/gl_shadow.py with the two things its loop cannot be given from outside:
the perturbed data fetch of R8kVolRen3D_cpy (volShadow binds the noise texture in BOTH passes and feeds both octaves'
scaled coordinates, :1566-1601; setupPBuff picks the perturbation shader for the light-space pass, :1125-1149) and the
sub-box of renderVolume(.., xext, yext, zext).  TEST INFRASTRUCTURE ONLY.

gl_shadow.render_shadow fetches at g.to_voxel(X) inside its slice loop, so the loop is restated here around gl_shadow's own
helpers (_Setup, _solve_on_plane, _raster, _tex3, _bilinear_border0, the flags), imported unchanged:

  * displaced fetch: a fragment exists, or not, by its own position X on the slice polygon (box, clip planes, the light
    buffer position, the depth); the volume, its normals and so the classification are fetched at
        tc' = tc + sum_q w_q (noise(tc s_q) - .5),   tc = X / fSize,   q = the two octaves the shader has,
    the noise texture GL_LINEAR / GL_REPEAT, u8 / 255, three channels -> three axes (R8kVolRen3D_cpy.cpp:3462-3490);
  * sub-box: sc.region = (g0, g1) in voxels (oracle.Scene's field), the model-space box g0 / N fSize .. g1 / N fSize
    intersected into the sliced box exactly as an orthogonal clip plane is -- the slice set stays the whole volume's.

With zero weights and the full region every array of the result equals render_shadow's, bit for bit
(tests/test_shadow_pert_ref.py)."""
import numpy as np

import gl_shadow
from gl_shadow import DELTA, _bilinear_border0, _raster, _Setup, _solve_on_plane, _tex3


def noise3(noise, tc):
    """GL_LINEAR, GL_REPEAT fetch of noise [r][t][s][>=3] u8 at texture coordinates tc [..., 3] (s, t, r) -> [..., 3]"""
    n = noise.shape[0]
    T = noise[..., :3].astype(np.float64) / 255.0
    u = tc * n - 0.5
    fl = np.floor(u)
    f = u - fl
    i0 = np.mod(fl.astype(np.int64), n)
    i1 = np.mod(i0 + 1, n)
    out = 0.0
    for zi, wz in ((i0[..., 2], 1 - f[..., 2]), (i1[..., 2], f[..., 2])):
        for yi, wy in ((i0[..., 1], 1 - f[..., 1]), (i1[..., 1], f[..., 1])):
            for xi, wx in ((i0[..., 0], 1 - f[..., 0]), (i1[..., 0], f[..., 0])):
                out = out + (wz * wy * wx)[..., None] * T[zi, yi, xi]
    return out


def perturbed(sc):
    return sc.noise is not None and any(float(w) != 0 for w in sc.pert_w[:2])


def displaced(g, p):
    """voxel coordinates p [..., 3] -> where the data is fetched"""
    sc = g.sc
    if not perturbed(sc):
        return p
    tc = (p + 0.5) / g.N
    o = np.zeros_like(tc)
    for q in range(2):
        w = float(sc.pert_w[q])
        if w != 0:
            o = o + w * (noise3(sc.noise, tc * float(sc.pert_s[q])) - 0.5)
    return (tc + o) * g.N - 0.5


def lipschitz(sc):
    """K of |p'(a) - p'(b)| <= K |a - b| per axis sum: 1 + sum_q w_q s_q n g, g the largest step between adjacent noise texels
    (wrap-around included), per channel, / 255 -- a trilinear texture's slope along an axis is at most one texel step per
    texel, there are n texels per unit coordinate and s_q units per unit tc"""
    if not perturbed(sc):
        return 1.0
    t = sc.noise[..., :3].astype(np.float64) / 255.0
    g = max(np.abs(t - np.roll(t, 1, axis=a)).max() for a in range(3))
    n = sc.noise.shape[0]
    return 1.0 + sum(abs(float(sc.pert_w[q])) * abs(float(sc.pert_s[q])) for q in range(2)) * n * g


def _setup(sc, delta):
    g = _Setup(sc, delta)
    r0, r1 = sc.region
    full = tuple(r0) == (0, 0, 0) and tuple(r1) == tuple(sc.dims)
    if not full:
        lo, hi = g.blo.copy(), g.bhi.copy()
        for a in range(3):
            lo[a] = max(lo[a], float(r0[a]) / g.N[a] * g.f[a])
            hi[a] = min(hi[a], float(r1[a]) / g.N[a] * g.f[a])
        g.blo, g.bhi = lo, hi
        g.box = np.array([[hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]] for i in range(8)])
        g.vlo, g.vhi = g.to_voxel(lo), g.to_voxel(hi)
    return g


def render_shadow(sc, delta=DELTA):
    """gl_shadow.render_shadow's frame and dict, with the displaced fetch and the sub-box"""
    g = _setup(sc, delta)
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

    def fetch_at(X):
        return displaced(g, g.to_voxel(X))

    for k in range(1, S + 1):
        c = g.plane(k)
        poly = g.polygon(c)
        # ---- eye pass: reads L as slices 1..k-1 left it
        Xd = _solve_on_plane(g.PM, g.eye_win, pxc, pyc, g.sn, c)
        fl = g.flags(Xd)
        if fl.any():
            amb |= fl
            bound[fl] = np.maximum(bound[fl], g.classify(_tex3(g.vol, fetch_at(Xd[fl])))[:, 3])
        if poly is not None:
            cov, X = _raster(g.PM, g.eye_win, poly, W, H)
            cov &= g.kept(X)
            if cov.any():
                Xs = X[cov]
                p = fetch_at(Xs)                            # (data and normal; everything else is Xs's)
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
                zeye = -(Xs @ g.MV[2, :3] + g.MV[2, 3])
                dp = depth[idx]
                depth[idx] = np.where(live, np.minimum(dp, zeye), dp)
        # ---- light pass: slice k composited onto L
        Xl = _solve_on_plane(g.LT, g.light_win, txc, tyc, g.sn, c)
        fl = g.flags(Xl)
        if fl.any():
            lamb |= fl
            lbound[fl] = np.maximum(lbound[fl], g.classify(_tex3(g.vol, fetch_at(Xl[fl])))[:, 3])
        if poly is not None:
            cov, X = _raster(g.LT, g.light_win, poly, LB, LB)
            cov &= g.kept(X)
            if cov.any():
                Xs = X[cov]
                col = g.classify(_tex3(g.vol, fetch_at(Xs)))
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


# ---- the scenes of tests/test_gpu_shadow_perturb.py, chosen on the CPU (tests/test_shadow_pert_ref.py holds each to the
# ambiguity caps of tests/test_shadow_witness.py on the reference alone), and their witnesses, computed once per process

def pert_scene(kind, light, pose, noise_n=32, region=None, pert=True, **kw):
    import oracle as O
    from test_shadow_witness import _scene
    sc = _scene(kind, light, pose, **kw)
    if pert:
        sc.noise = O.noise_tex(noise_n)
        sc.pert_w = (.2, .1, 0, 0)
        sc.pert_s = (.2, 2.1, 4.5, 8.7)
    if region is not None:
        sc.region = region
    return sc


# (name: kind, light, pose, arguments) -- the issue's table, the ragged case and the 24^3 noise texture
CASES = {
    "cfg3-u8-shade-oblique-rot": ("cfg3", "oblique", "rot", dict(shade=1)),
    "cfg3-f32-shade-behind-back": ("cfg3", "behind", "back", dict(f32=True, shade=1)),
    "cfg3-f32-flat-eye_side-id": ("cfg3", "eye_side", "id", dict(f32=True, shade=0)),
    "cfg2-third-shade-side-side": ("cfg2", "side", "side", dict(shade=1)),
    "tf3d-flat-oblique-id": ("tf3d", "oblique", "id", dict(shade=0)),
    "ragged": ("cfg3", "side", "rot", dict(dims=(40, 24, 18), size=45, shade=1, shadow=(70, 0.5), steps=0, sample_rate=1.5)),
    "noise24": ("cfg3", "oblique", "rot", dict(f32=True, shade=1, noise_n=24)),
}
REGION = ((6, 0, 0), (32, 25, 32))          # cut on two axes: x from below, y from above
SUBBOX_CASES = {
    "region": ("cfg3", "oblique", "rot", dict(f32=True, shade=1, region=REGION, pert=False)),
    "region-pert": ("cfg3", "oblique", "rot", dict(f32=True, shade=1, region=REGION)),
    "region-free-plane": ("cfg3", "oblique", "rot", dict(f32=True, shade=1, region=REGION, pert=False, free_plane=True)),
}


def case_scene(name, pert=None):
    kind, light, pose, kw = {**CASES, **SUBBOX_CASES}[name]
    kw = dict(kw)
    sample_rate = kw.pop("sample_rate", None)
    free_plane = kw.pop("free_plane", False)
    if pert is not None:
        kw["pert"] = pert
    sc = pert_scene(kind, light, pose, **kw)
    if sample_rate is not None:
        sc.sample_rate = sample_rate
    if free_plane:
        n = np.array([0.35, -0.2, -0.9])
        n /= np.linalg.norm(n)
        mv = np.array(sc.mv(), np.float64).reshape(4, 4).T
        centre = mv @ np.array([float(sc.fsize[0]) / 2, float(sc.fsize[1]) / 2, float(sc.fsize[2]) / 2, 1.0])
        sc.clip_plane = (n[0], n[1], n[2], -float(n @ centre[:3]) + 0.03)
    return sc


_WITNESS = {}


def witness(name, pert=None):
    """(scene, reference dict) of a named case; read-only, shared by the tests of a process"""
    key = (name, pert)
    if key not in _WITNESS:
        sc = case_scene(name, pert)
        w = render_shadow(sc)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WITNESS[key] = (sc, w)
    return _WITNESS[key]


def region_extents(sc):
    """sc.region (voxels) as smk_set_region takes it: volume-space lo, hi"""
    r0, r1 = sc.region
    f = [float(v) for v in sc.fsize]
    return ([r0[a] / sc.dims[a] * f[a] for a in range(3)], [r1[a] / sc.dims[a] * f[a] for a in range(3)])
