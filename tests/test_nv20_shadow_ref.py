"""The float64 reference of the NV20 shadow look (tests/_nv20_shadow_ref.py) tied to the code that exists: its light side to
oracle/gl_shadow.py bit for bit, its eye fragment to gl_shadow's through a white table (where the light buffer's colour and
opacity obey the same recurrence) and to the C checker's unshadowed frames through amb = 1 (where the shadow weight is 1 and
a light on the view axis makes the half-angle slices the view-aligned ones).  tests/test_gpu_shadow_nv20.py trusts this
reference.  Runs without a GPU.

Bounds: TOL, AMB_CAP, LAMB_CAP of tests/test_shadow_witness.py -- the same comparison class as there, a float64 pipeline
against the fp32 checker."""
import numpy as np
import pytest

import _nv20_shadow_ref as N
from test_shadow_witness import AMB_CAP, LAMB_CAP, LTOL, TOL, _scene

MASKS = ("amb", "lamb", "lamb_history", "bound", "lbound")
# (kind, light, pose) -- unshaded, so that gl_shadow.render_shadow draws the same scene in the R8k look
LIGHT_SIDE = [("cfg3", "oblique", "rot"), ("cfg2", "eye_side", "rot"), ("tf3d", "side", "back"), ("cfg3", "behind", "back")]
_IDS = ["-".join(c) for c in LIGHT_SIDE]
_R8K = {}


def _r8k(case):
    """gl_shadow.render_shadow of an unshaded case: the R8k look's frame, the light side both looks share"""
    import gl_shadow
    if case not in _R8K:
        _R8K[case] = gl_shadow.render_shadow(_scene(*case, shade=0))
    return _R8K[case]


def _nv20(case, amb):
    return N.witness_of(("ref",) + case + (amb,), lambda: N.nv20_scene(*case, shade=0, amb=amb))[1]


@pytest.mark.parametrize("case", LIGHT_SIDE, ids=_IDS)
def test_light_side_untouched(O, case):
    w, r = _nv20(case, 0.0), _r8k(case)
    assert w["nslices"] == r["nslices"] and w["front_to_back"] == r["front_to_back"]
    for key in ("light", "history", "depth") + MASKS:
        assert np.array_equal(w[key], r[key]), key


def test_white_table_makes_the_two_looks_one(O):
    """colour 1 everywhere: L.rgb <- a + (1 - a) L.rgb is L.a's recurrence, so 1 - L.rgb = 1 - L.a (1 - 0)"""
    import gl_shadow

    def white(sc):
        sc.tf_vg = sc.tf_vg.copy()
        sc.tf_vg[..., :3] = 255
        return sc
    r = gl_shadow.render_shadow(white(_scene("cfg2", "oblique", "rot", shade=0)))
    w = N.render_shadow(white(N.nv20_scene("cfg2", "oblique", "rot", shade=0, amb=0.0)))
    assert r["rgba"][..., 3].max() > 0.05 and r["light"][..., 3].max() > 0.05
    assert np.array_equal(w["rgba"], r["rgba"]), np.abs(w["rgba"] - r["rgba"]).max()


@pytest.mark.parametrize("kind,pose,shade", [("cfg3", "id", 0), ("cfg3", "rot", 0), ("cfg2", "rot", 0), ("cfg3", "rot", 2), ("cfg3", "id", 2)],
                         ids=["cfg3-id", "cfg3-rot", "cfg2-rot", "cfg3-rot-nv20", "cfg3-id-nv20"])
def test_amb_one_on_the_view_axis_is_the_checkers_unshadowed_frame(O, kind, pose, shade):
    sc = N.nv20_scene(kind, "eye_side", pose, shade=shade, amb=1.0)
    w = N.render_shadow(sc)
    ref = sc.render()                       # (the C checker: view-aligned slices, no shadows, NV20 Phong where shade = 2)
    assert ref[..., 3].max() > 0.05
    d = np.abs(w["rgba"] - ref).max()
    print(f"{kind} {pose} shade {shade}: max abs difference {d:.3g}")
    assert d <= TOL, d


def test_amb_acts_on_colour_alone(O):
    case = ("cfg3", "oblique", "rot")
    frames = [_nv20(case, amb)["rgba"] for amb in (0.0, 0.05, 0.5, 1.0)]
    for a, b in zip(frames, frames[1:]):
        assert np.array_equal(a[..., 3], b[..., 3])
        assert (b[..., :3] >= a[..., :3]).all()
    assert np.abs(frames[-1][..., :3] - frames[0][..., :3]).max() > 0.05


@pytest.mark.parametrize("case", LIGHT_SIDE, ids=_IDS)
def test_not_vacuous(O, case):
    """a kernel that reads the light buffer's colour, or drops 1 - amb, is far outside TOL on most of the frame"""
    w0, w05, w1, r = _nv20(case, 0.0), _nv20(case, 0.05), _nv20(case, 1.0), _r8k(case)
    cov = r["rgba"][..., 3] > 0
    far = np.abs(w0["rgba"] - r["rgba"]).max(axis=2) > 10 * TOL
    print(f"look 1 at amb 0 against look 0: {(far & cov).sum()} of {cov.sum()} covered pixels differ")
    assert (far & cov).sum() >= 0.5 * cov.sum()
    far = np.abs(w05["rgba"] - w1["rgba"]).max(axis=2) > 10 * TOL
    print(f"amb .05 against amb 1: {(far & cov).sum()} of {cov.sum()} covered pixels differ")
    assert (far & cov).sum() >= 0.5 * cov.sum()


@pytest.mark.parametrize("case", LIGHT_SIDE, ids=_IDS)
def test_ambiguity_caps(O, case):
    w = _nv20(case, 0.0)
    cov = w["rgba"][..., 3] > 0
    assert cov.sum() >= 50
    assert (w["amb"] & cov).sum() <= AMB_CAP * cov.sum()
    assert w["lamb"].mean() <= LAMB_CAP


@pytest.mark.parametrize("name", sorted(N.CASES))
def test_gpu_cases_qualify_on_the_cpu(O, name):
    """the scenes of tests/test_gpu_shadow_nv20.py: the C checker's light buffer (fp32, the product's arithmetic; the look
    does not touch the light side) within LTOL of this reference's on unambiguous texels, the ambiguity caps, not vacuous"""
    sc, w = N.witness(name)
    _, refL = N.case_scene(name, shade=0).render_shadow()
    cov = w["rgba"][..., 3] > 0
    assert w["rgba"][..., 3].max() > 0.05 and w["light"][..., 3].max() > 0.05 and cov.sum() >= 50
    assert (w["amb"] & cov).sum() <= AMB_CAP * cov.sum() and w["lamb"].mean() <= LAMB_CAP
    d = np.abs(refL - w["light"]).max(axis=2)[~w["lamb"]].max()
    print(f"{name}: checker light buffer against the reference, unambiguous texels: {d:.3g}")
    assert d <= LTOL
