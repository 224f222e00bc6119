"""The shadow checker (oracle/smk_oracle.c orc_shadow_setup / orc_render_shadow) against an independent witness: the
half-angle GL slice pipeline restated in float64 (oracle/gl_shadow.py).  The checker's eye pass is the product's fma chain
and its light rays the product's, so these tests are what would notice a misreading the two share.  Runs without a GPU.

Bounds (tests/test_gpu_shadow_witness.py holds the product to the same ones):
  * delta: a sample up to 2e-3 voxels outside or 1e-4 inside a box face, or 2e-3 from a free clip plane, is ambiguous.
    The checker takes every sample within 2^-10 voxels of the box (a face-coincident slice must be drawn), GL does not:
    2e-3 covers that band plus the fp32 placement error; the placement error alone (< 5e-5, PLACEMENT) is below 1e-4.
  * a pixel or texel that is not ambiguous agrees to 4e-4 (TOL); an ambiguous one differs by at most one slice's contribution
    (the largest alpha among its own samples).
  * at most AMB_CAP of the covered pixels and LAMB_CAP of the texels are ambiguous, and the scene is not vacuous.
"""
import numpy as np
import pytest

from _scenes import make_scene

TOL = 4e-4            # fp32 vs float64: every sample's fetch error times the slope of an 8-bit table ramp (the cfg 3
LTOL = TOL            # triangle widget rises by one unit per texel = 255 per unit value), accumulated over the slices
PLACEMENT = 1e-4      # voxels: the checker's chain (fp32 coefficients) evaluated in float64 vs the direct intersection
AMB_CAP = 0.35        # of the covered pixels: a flagged light texel taints every later eye sample that reads it
LAMB_CAP = 0.03       # of the texels
LIGHTS = {"eye_side": (0, 0, -5), "oblique": (3, 4, -3), "behind": (-2, 3, 4), "side": (5, 1, 0.5),
          "perp_front": (5, 0.3, -0.05), "perp_back": (5, 0.3, 0.05)}     # v.l just above / below 0


def _scene(kind, light, pose="rot", n=32, size=48, steps=40, shadow=(64, 0.5), **kw):
    third = kw.pop("third", kind == "cfg2")
    sc = make_scene(kind, n=n, size=size, steps=steps, pose=pose, third=third, **kw)
    sc.light_pos = LIGHTS[light] if isinstance(light, str) else light
    sc.shadow = shadow
    return sc


def compare(got, gotL, w, tol=TOL, ltol=LTOL, exact=False):
    """frame [H][W][4] and light buffer [LB][LB][4] against the witness dict w"""
    assert gotL.shape == w["light"].shape
    cov = w["rgba"][..., 3] > 0
    assert w["rgba"][..., 3].max() > 0.05 and w["light"][..., 3].max() > 0.05, "vacuous scene"
    amb, lamb = (np.zeros_like(w["amb"]), np.zeros_like(w["lamb"])) if exact else (w["amb"], w["lamb"])
    assert (cov & ~amb).sum() >= 0.2 * cov.sum() and cov.sum() >= 50, "vacuous scene"
    assert (amb & cov).sum() <= AMB_CAP * cov.sum(), f"{(amb & cov).sum()} of {cov.sum()} pixels ambiguous"
    assert lamb.mean() <= LAMB_CAP, f"{lamb.sum()} texels ambiguous"
    d = np.abs(got - w["rgba"]).max(axis=2)
    dl = np.abs(gotL - w["light"]).max(axis=2)
    assert d[~amb].max(initial=0) <= tol, f"frame: {(d[~amb] > tol).sum()} unambiguous pixels differ, max {d[~amb].max()}"
    assert dl[~lamb].max(initial=0) <= ltol, f"light: {(dl[~lamb] > tol).sum()} unambiguous texels differ, max {dl[~lamb].max()}"
    assert (d[amb] <= w["bound"][amb] + tol).all(), "an ambiguous pixel differs by more than one slice"
    assert (dl[lamb] <= w["lbound"][lamb] + ltol).all(), "an ambiguous texel differs by more than one slice"


CASES = [
    # (kind, light, pose, extra make_scene arguments)
    ("cfg3", "eye_side", "id", dict(shade=1)),
    ("cfg3", "oblique", "rot", dict(shade=1)),
    ("cfg3", "behind", "back", dict(shade=1)),
    ("cfg3", "side", "side", dict(shade=1)),
    ("cfg3", "perp_front", "rot", dict(shade=1)),
    ("cfg3", "perp_back", "rot", dict(shade=1)),
    ("cfg3", "oblique", "side", dict(f32=True, shade=1)),
    ("cfg3", "eye_side", "rot", dict(f32=True, shade=0)),
    ("cfg3", "behind", "id", dict(f32=True, shade=1)),
    ("cfg2", "eye_side", "rot", dict(shade=0)),
    ("cfg2", "oblique", "back", dict(shade=1)),
    ("cfg2", "perp_back", "side", dict(shade=0)),
    ("tf3d", "oblique", "id", dict(shade=0)),
    ("tf3d", "behind", "rot", dict(shade=1)),
    ("tf3d", "side", "back", dict(shade=0)),
    ("tf3d", "perp_front", "side", dict(shade=1, n=24, size=32, steps=30)),
]


@pytest.mark.parametrize("kind,light,pose,kw", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{i}" for i, c in enumerate(CASES)])
def test_checker_frame_and_light_buffer_equal_the_witness(O, kind, light, pose, kw):
    import gl_shadow
    sc = _scene(kind, light, pose, **dict(kw))
    w = gl_shadow.render_shadow(sc)
    c = sc.shadowcoef()
    assert bool(c.front_to_back) == w["front_to_back"] and c.nslices == w["nslices"] and c.LB == w["light"].shape[0]
    ref, refL = sc.render_shadow()
    compare(ref, refL, w)


def test_near_perpendicular_lights_flip_the_order(O):
    import gl_shadow
    f = gl_shadow.render_shadow(_scene("cfg3", "perp_front", n=24, size=32, steps=24))
    b = gl_shadow.render_shadow(_scene("cfg3", "perp_back", n=24, size=32, steps=24))
    assert f["front_to_back"] and not b["front_to_back"]


def test_ragged_volume_sample_rate_mode_odd_viewport(O):
    import gl_shadow
    sc = _scene("cfg3", "side", "rot", dims=(40, 24, 18), size=45, shade=1, shadow=(64, 1.0))
    sc.steps, sc.sample_rate = 0, 1.5
    w = gl_shadow.render_shadow(sc)
    assert w["nslices"] == sc.shadowcoef().nslices
    compare(*sc.render_shadow(), w)


@pytest.mark.parametrize("which", ["orthogonal", "free"])
def test_clip_planes(O, which):
    import gl_shadow
    sc = _scene("cfg3", "oblique", "rot", f32=True, shade=1, shadow=(96, 0.7))
    if which == "orthogonal":
        sc.clip = (3, tuple(0.55 * float(f) for f in sc.fsize))
    else:
        n = np.array([0.35, -0.2, -0.9])
        n /= np.linalg.norm(n)
        mv = np.array(sc.mv(), np.float64).reshape(4, 4).T
        centre = mv @ np.array([float(sc.fsize[0]) / 2, float(sc.fsize[1]) / 2, float(sc.fsize[2]) / 2, 1.0])
        sc.clip_plane = (n[0], n[1], n[2], -float(n @ centre[:3]) + 0.03)
    w = gl_shadow.render_shadow(sc)
    compare(*sc.render_shadow(), w)


def _chain(c, W, H, k):
    """the checker's / the product's eye-sample chain (smk_ray_AB) on shadowcoef()'s fp32 coefficients, in float64"""
    px = np.float32(np.float32(np.arange(W) + 0.5) * np.float32(c.pxs) + np.float32(c.pxl)).astype(np.float64)[None, :]
    py = np.float32(np.float32(np.arange(H) + 0.5) * np.float32(c.pys) + np.float32(c.pyl)).astype(np.float64)[:, None]
    S = c.nslices
    numA = (c.dnum + c.num0) if c.front_to_back else (S * c.dnum + c.num0)
    dB = c.dnum if c.front_to_back else -c.dnum
    m = k - 1 if c.front_to_back else S - k
    nD = px * c.nDx + py * c.nDy + c.nDc
    tauA, dtau = numA / nD, dB / nD
    return np.stack([tauA * (px * c.Dx[a] + py * c.Dy[a] + c.Dc[a]) + c.Ec[a]
                     + m * dtau * (px * c.Dx[a] + py * c.Dy[a] + c.Dc[a]) for a in range(3)], axis=-1)


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("pose,dims,steps", [("rot", None, 40), ("side", (40, 24, 18), 0)])
def test_placement_of_the_eye_chain(O, light, pose, dims, steps):
    """A + m B of slice k lies on the plane the witness rasterises for slice k, at the pixel ray's direct intersection"""
    import gl_shadow
    sc = _scene("cfg3", light, pose, dims=dims, steps=steps, size=37)
    if not steps:
        sc.sample_rate = 1.3
    c = sc.shadowcoef()
    S = c.nslices
    for k in (1, S // 2, S):
        p, g = gl_shadow.eye_samples(sc, k)
        q = _chain(c, sc.width, sc.height, k)
        err = np.abs(p - q).max()
        assert err <= PLACEMENT, f"slice {k}: chain vs intersection {err} voxels"
        X = (q + 0.5) / g.N * g.f
        assert np.abs(X @ g.sn - g.plane(k)).max() / g.dc < 1e-3       # (on slice k's plane, not a neighbour's)


def test_light_history_closed_form(O):
    """homogeneous volume, light on the view axis, axis-aligned pose: every slice covers the centre texel, whose alpha
    after k slices is 1 - (1 - a)^k (R8kVolRen3D.cpp:3158-3162)"""
    import gl_shadow
    sc = O.Scene(np.full((24, 24, 24, 2), 128, np.uint8))
    tf = np.zeros((16, 16, 4), np.uint8)
    tf[..., 0], tf[..., 1], tf[..., 2], tf[..., 3] = 204, 102, 51, 26
    sc.tf_mode, sc.tf_vg = 1, tf
    sc.width = sc.height = 24
    sc.steps = 30
    sc.shadow = (64, 0.5)
    w = gl_shadow.render_shadow(sc)
    a = 26 / 255
    c = w["light"].shape[0] // 2
    for k in (1, 15, 30):
        assert abs(w["history"][k][c, c, 3] - (1 - (1 - a) ** k)) <= 1e-12
    assert not w["history"][0].any() and np.array_equal(w["history"][30], w["light"])
    assert np.abs(w["light"] - sc.render_shadow()[1]).max() <= TOL


def face_scene(O):
    """steps mode, light on the view axis, identity pose: h = +z and the last slice (k = S) lies ON the far face z = fz,
    where an opaque layer sits"""
    n = 32
    data = np.zeros((n, n, n, 2), np.uint8)
    data[..., 0] = 40
    data[..., 1] = 128
    data[-1, ..., 0] = 255
    sc = O.Scene(data)
    tf = np.zeros((16, 16, 4), np.uint8)
    tf[..., :3] = (200, 150, 100)
    tf[..., 3] = 8
    tf[:, 12:, 3] = 255                      # the face's value is opaque
    sc.tf_mode, sc.tf_vg = 1, tf
    sc.width = sc.height = 36
    sc.steps = 30
    sc.light_pos = (0, 0, -3.3)
    sc.shadow = (64, 0.5)
    return sc


def test_face_coincident_last_slice(O):
    """GL rasterises the slice polygon that lies on a face, so the witness draws slice S in both passes.  No ambiguity
    allowance: every pixel and texel matches.  (The checker's light pass once tested a closed box while its eye pass took
    the box 2^-10 voxels wide: the light samples of slice S fell outside by rounding and the final light buffer missed the
    opaque face -- 0.4 on every lit texel of this scene.)"""
    import gl_shadow
    sc = face_scene(O)
    w = gl_shadow.render_shadow(sc)
    S = w["nslices"]
    assert abs(w["planes"][0] + S * w["planes"][1] - float(sc.fsize[2])) < 1e-12
    lit = w["history"][S][..., 3] - w["history"][S - 1][..., 3]
    assert (lit > 0.3).sum() >= 100             # the last slice is drawn into the light buffer, opaque
    compare(*sc.render_shadow(), w, exact=True)
