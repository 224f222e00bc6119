"""The float64 half-angle slice pipeline of oracle/gl_shadow.py in the NV20 look (option shadow_look 1): what the fourth
renderer of the reference, NV20VolRen3D2, draws when gluvv.light.shadow is on -- as this project builds it (DESIGN.md
section 8 lists where that departs from the class as coded).  TEST INFRASTRUCTURE ONLY.

gl_shadow.render_shadow's eye fragment is the R8k one and sits inside its slice loop, so the loop is restated here around
gl_shadow's own helpers (_Setup, _solve_on_plane, _raster, _tex3, _bilinear_border0, the flags), imported unchanged, as
tests/_shadow_pert_ref.py does.  Two things differ:

  * the eye fragment looks the light buffer's OPACITY up, L[..., 3] (NV20VolRen3D2::setupRegComb reads the shadow texture's
    alpha, :866-945), where the R8k fragment looks up L[..., :3];
  * the fragment's colour: with La that lookup, f = 1 - sat(La) (1 - amb), amb = gluvv.light.amb (CONSTANT_COLOR1.a =
    1 - amb), shading off gives sat(c f a) and alpha a; NV20 Phong gives r f and alpha a, r the six combiners of
    NV20VolRen3D::setupRegComb (NV20VolRen3D.cpp:634-806) restated below.  The shadow never touches alpha.

The light pass, the history, the ambiguity masks and the bounds are render_shadow's: they depend on geometry and opacity
alone (tests/test_nv20_shadow_ref.py holds them equal, bit for bit)."""
import numpy as np

import gl_shadow
from gl_shadow import DELTA, _bilinear_border0, _raster, _Setup, _solve_on_plane, _tex3

AMB_DEFAULT = 0.05        # gluvv.light.amb as initGluvv leaves it (gluvv.cpp:293)


def keep_of(amb):
    """1 - amb as the library computes it: one fp32 subtraction"""
    return float(np.float32(1.0) - np.float32(amb))


def nv20_vectors(g):
    """light and half-way direction of the NV20 combiners in the volume's space (NV20VolRen3D.cpp:637-668): ltdir =
    norm(light.pos - at), vdir = norm(eye - at), half = ltdir + (vdir - ltdir) / 2, both through the inverse of rinfo.xform
    (a rotation), negated, normalised"""
    sc = g.sc
    at = np.asarray(sc.at, np.float64)
    vd = np.asarray(sc.eye, np.float64) - at
    vd /= np.linalg.norm(vd)
    lt = np.asarray(sc.light_pos, np.float64) - at
    lt /= np.linalg.norm(lt)
    half = lt + 0.5 * (vd - lt)
    Rinv = np.linalg.inv(g.xf[:3, :3])
    hv, lv = -(Rinv @ half), -(Rinv @ lt)
    return lv / np.linalg.norm(lv), hv / np.linalg.norm(hv)


def nv20_phong(g, p, col, Lv, Hv):
    """the six general combiners and the final one: premultiplied rgb of straight colour col [..., 4] at voxel position p"""
    sc = g.sc
    a = col[..., 3:4]
    c = col[..., :3]
    n = _tex3(g.grad, p) * (2.0 / 255.0) - 1.0              # GL_EXPAND_NORMAL of the normal texture
    dl = np.abs(n @ Lv)[..., None]                          # combiners 1-2: N.L and -N.L, unsigned, summed
    dh = (n @ Hv)[..., None]
    s16 = np.clip(dh * dh, 0, 1) ** 8                       # combiners 1-4 (alpha): (N.H)^2 of either side, squared three times
    ia, aa = float(sc.intens) * a, 0.3 * a                  # combiner 2: light intensity x alpha; combiner 3: ambient .3 x alpha
    cc = np.clip(c * np.clip(dl, 0, 1) * ia + c * aa, 0, 1)  # combiner 4: diffuse and ambient
    spec = s16 * ia if sc.use_spec else 0.0 * ia            # combiner 5 (gluvvShadeDiff: no specular term)
    return np.clip(spec * (1.0 - cc) + cc, 0, 1)            # final combiner: A B + (1 - A) C + D


def render_shadow(sc, delta=DELTA):
    """gl_shadow.render_shadow's frame and dict in the NV20 look; sc.amb = gluvv.light.amb (default .05), sc.shade_mode 0
    or 2"""
    if sc.shade_mode not in (0, 2):
        raise ValueError("the NV20 look takes shading off or the NV20 form")
    g = _Setup(sc, delta)
    keep = keep_of(getattr(sc, "amb", AMB_DEFAULT))
    shaded = sc.shade_mode == 2 and g.grad is not None
    if shaded:
        Lv, Hv = nv20_vectors(g)
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
        if fl.any():
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
                La, taps = _bilinear_border0(L[..., 3:4], lx, ly)       # (the shadow texture's alpha)
                f = 1.0 - np.clip(La, 0, 1) * keep
                a = col[..., 3]
                if shaded:
                    rgb = nv20_phong(g, p, col, Lv, Hv) * f
                else:
                    rgb = np.clip(col[..., :3] * f * a[..., None], 0, 1)
                src = np.concatenate([rgb, a[..., None]], axis=-1)
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
        # ---- light pass: slice k composited onto L (render_shadow's, unchanged)
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


# ---- the scenes of tests/test_gpu_shadow_nv20.py, chosen on the CPU (tests/test_nv20_shadow_ref.py holds the reference
# to the ambiguity caps of tests/test_shadow_witness.py on them), and their witnesses, computed once per process

def nv20_scene(kind, light, pose, amb=AMB_DEFAULT, sample_rate=None, spec=True, **kw):
    from test_shadow_witness import _scene
    sc = _scene(kind, light, pose, **kw)
    sc.amb = amb
    sc.use_spec = 1 if spec else 0
    if sample_rate is not None:
        sc.steps, sc.sample_rate = 0, sample_rate
    return sc


# name: (kind, light, pose, arguments).  shade 0 = none, 2 = NV20 Phong (spec=False: diffuse alone).  Every table kind, both
# voxel types, the six lights of test_shadow_witness.LIGHTS, four poses, the third axis on (cfg2, cfg4) and off, amb 0 / .05 / .5
# A case qualifies on the CPU, before any GPU sees it: the light buffer -- which the look does not touch -- of the fp32 C
# checker lies within LTOL of this float64 pipeline on the unambiguous texels, and the ambiguity caps hold
# (tests/test_nv20_shadow_ref.py::test_gpu_cases_qualify_on_the_cpu).  The grazing light perp_back with FLOAT voxels does not:
# the checker's own light buffer is 4.5e-4 from the float64 one on one texel of cfg 3's steep table ramp (the fp32 recurrence
# over 40 slices; tests/test_gpu_shadow_witness.py notes 5.2e-4 on mid-frame buffers of cfg 3 f32), so that light is paired
# with byte voxels here, as tests/test_shadow_witness.py pairs it.
CASES = {
    "cfg3-u8-dspec-oblique-rot-amb.05": ("cfg3", "oblique", "rot", dict(shade=2)),
    "cfg3-f32-dspec-behind-back-amb.5": ("cfg3", "behind", "back", dict(f32=True, shade=2, amb=0.5)),
    "cfg3-f32-none-eye_side-id-amb0": ("cfg3", "eye_side", "id", dict(f32=True, shade=0, amb=0.0)),
    "cfg3-u8-diff-side-side-amb0": ("cfg3", "side", "side", dict(shade=2, spec=False, amb=0.0)),
    "cfg3-u8-none-perp_front-rot-amb.05": ("cfg3", "perp_front", "rot", dict(shade=0)),
    "cfg3-u8-dspec-perp_back-rot-amb.05": ("cfg3", "perp_back", "rot", dict(shade=2)),
    "cfg2-u8-third-none-eye_side-rot-amb.5": ("cfg2", "eye_side", "rot", dict(shade=0, amb=0.5)),
    "cfg2-u8-nothird-dspec-oblique-back-amb0": ("cfg2", "oblique", "back", dict(shade=2, third=False, amb=0.0)),
    "cfg4-f32-third-diff-behind-side-amb.05": ("cfg4", "behind", "side", dict(f32=True, shade=2, spec=False)),
    "tf3d-u8-none-side-back-amb0": ("tf3d", "side", "back", dict(shade=0, amb=0.0)),
    "tf3d-f32-dspec-oblique-id-amb.5": ("tf3d", "oblique", "id", dict(f32=True, shade=2, amb=0.5)),
    "ragged-u8-dspec-side-rot-amb.05": ("cfg3", "side", "rot", dict(dims=(40, 24, 18), size=45, shade=2, shadow=(64, 1.0), sample_rate=1.5)),
    "ragged-light-f32-none-oblique-rot-amb.05": ("cfg3", "oblique", "rot", dict(f32=True, shade=0, shadow=(96, 0.7))),
}


def case_scene(name, **over):
    kind, light, pose, kw = CASES[name]
    return nv20_scene(kind, light, pose, **{**kw, **over})


_WITNESS = {}


def witness_of(key, make):
    """(scene, reference dict) under `key`, made once per process by make() -> scene; read-only"""
    if key not in _WITNESS:
        sc = make()
        w = render_shadow(sc)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WITNESS[key] = (sc, w)
    return _WITNESS[key]


def witness(name):
    return witness_of(name, lambda: case_scene(name))
