"""The float64 reference of perturbed and sub-box frames with shadows (tests/_shadow_pert_ref.py) against the witness it
restates (oracle/gl_shadow.py), and the conditions its scenes must meet before tests/test_gpu_shadow_perturb.py may
hold the product to them.  Runs without a GPU."""
import numpy as np
import pytest

import _shadow_pert_ref as ref
from test_shadow_witness import AMB_CAP, LAMB_CAP, TOL, _scene

ARRAYS = ("rgba", "light", "history", "depth", "amb", "lamb", "lamb_history", "bound", "lbound")


def _same(a, b, keys=ARRAYS):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key
    assert a["front_to_back"] == b["front_to_back"] and a["nslices"] == b["nslices"]


@pytest.mark.parametrize("kind,light,pose,kw", [("cfg3", "oblique", "rot", dict(f32=True, shade=1)),
                                                ("tf3d", "behind", "back", dict(shade=0))])
def test_zero_weights_and_the_full_region_are_the_witness_itself(O, kind, light, pose, kw):
    import gl_shadow
    sc = _scene(kind, light, pose, **kw)
    want = gl_shadow.render_shadow(sc)
    sc.noise = O.noise_tex(32)
    sc.pert_w = (0, 0, 0, 0)
    _same(ref.render_shadow(sc), want)


@pytest.mark.parametrize("axis,upper,face", [(0, True, 20), (2, False, 9)])
def test_a_sub_box_that_moves_one_face_is_that_orthogonal_clip_plane(O, axis, upper, face):
    import gl_shadow
    sc = _scene("cfg3", "oblique", "rot", f32=True, shade=1)
    r0, r1 = [0, 0, 0], list(sc.dims)
    (r1 if upper else r0)[axis] = face
    sc.region = (tuple(r0), tuple(r1))
    got = ref.render_shadow(sc)
    sc.region = ((0, 0, 0), tuple(sc.dims))
    vpos = [0.0, 0.0, 0.0]
    vpos[axis] = float(face) / float(sc.dims[axis]) * float(sc.fsize[axis])
    sc.clip = (2 * axis + (1 if upper else 2), tuple(vpos))
    want = gl_shadow.render_shadow(sc)
    _same(got, want, ("rgba", "light", "history"))
    whole = gl_shadow.render_shadow(_scene("cfg3", "oblique", "rot", f32=True, shade=1))
    assert np.abs(whole["rgba"] - got["rgba"]).max() > 0.05           # (the sub-box IS another frame)


@pytest.mark.parametrize("name", sorted(ref.CASES) + ["region-pert"])
def test_the_perturbed_scenes_are_not_vacuous(O, name):
    """the perturbed frame and light buffer differ from their unperturbed twins by more than 20 x the tolerance the GPU
    test uses for them (K TOL), on at least a tenth of the covered pixels and texels"""
    sc, w = ref.witness(name)
    _, plain = ref.witness(name, pert=False)
    tol = ref.lipschitz(sc) * TOL
    cov = (w["rgba"][..., 3] > 0) | (plain["rgba"][..., 3] > 0)
    lcov = (w["light"][..., 3] > 0) | (plain["light"][..., 3] > 0)
    d = np.abs(w["rgba"] - plain["rgba"]).max(axis=2)
    dl = np.abs(w["light"] - plain["light"]).max(axis=2)
    assert cov.sum() >= 50 and lcov.sum() >= 50
    assert (d[cov] > 20 * tol).mean() >= 0.1, f"frame: {(d[cov] > 20 * tol).mean():.3f} of the covered pixels (K {ref.lipschitz(sc):.2f})"
    assert (dl[lcov] > 20 * tol).mean() >= 0.1, f"light: {(dl[lcov] > 20 * tol).mean():.3f} of the covered texels"


@pytest.mark.parametrize("name", sorted(ref.CASES) + sorted(ref.SUBBOX_CASES))
def test_ambiguity_caps_of_the_gpu_scenes(O, name):
    """conditions on the scenes, on the reference alone: what tests/test_shadow_witness.py::compare asserts of a witness"""
    sc, w = ref.witness(name)
    cov = w["rgba"][..., 3] > 0
    assert w["rgba"][..., 3].max() > 0.05 and w["light"][..., 3].max() > 0.05 and cov.sum() >= 50, "vacuous scene"
    assert (cov & ~w["amb"]).sum() >= 0.2 * cov.sum()
    assert (w["amb"] & cov).sum() <= AMB_CAP * cov.sum(), f"{(w['amb'] & cov).sum()} of {cov.sum()} pixels ambiguous"
    assert w["lamb"].mean() <= LAMB_CAP, f"{w['lamb'].sum()} texels ambiguous"
    assert w["light"].shape[0] == int(np.ceil(sc.shadow[0] * sc.shadow[1]))


def test_the_lipschitz_constant_bounds_the_displacement_map(O):
    """K = 1 + sum w_q s_q n g: finite differences of the displaced position, axis by axis, on random points"""
    sc = ref.case_scene("noise24")
    g = ref._setup(sc, 2e-3)
    K = ref.lipschitz(sc)
    rng = np.random.default_rng(7)
    p = rng.uniform(0, 31, (4000, 3))
    for a in range(3):
        q = p.copy()
        q[:, a] += 1e-3
        assert (np.abs(ref.displaced(g, q) - ref.displaced(g, p)).max(axis=1) <= K * 1e-3 * (1 + 1e-9)).all()
    assert K > 1.5
