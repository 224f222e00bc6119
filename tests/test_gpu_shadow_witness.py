"""The product's shadow frames, light buffers, per-slice light history and first-hit depth compared DIRECTLY with the
float64 half-angle slice pipeline (oracle/gl_shadow.py), under the bounds of tests/test_shadow_witness.py: the eye pass
on the gather kernel, on the slice-ring kernel and as a launch per slice (option shadow_march 0)."""
import numpy as np
import pytest

from _scenes import push_scene
from test_shadow_witness import CASES, TOL, _scene, compare, face_scene

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def _paths(R):
    """(frame, light buffer, renderer) for kernel 1, kernel 2 and a launch per slice"""
    out = []
    try:
        for kern in (1, 2):
            R.set_option("kernel", kern)
            out.append((R.render(), R.light_buffer()))
            assert R.last_frame_info()[0] == kern
        R.set_option("kernel", 0)
        R.set_option("shadow_march", 0)
        out.append((R.render(), R.light_buffer()))
        assert R.last_frame_info()[0] == 3
    finally:
        R.set_option("shadow_march", 1)
        R.set_option("kernel", 0)
    return out


@pytest.mark.parametrize("kind,light,pose,kw", CASES, ids=[f"{c[0]}-{c[1]}-{c[2]}-{i}" for i, c in enumerate(CASES)])
def test_frames_buffers_and_history_equal_the_witness(R, O, kind, light, pose, kw):
    import gl_shadow
    sc = _scene(kind, light, pose, **dict(kw))
    w = gl_shadow.render_shadow(sc)
    push_scene(R, sc)
    for got, gotL in _paths(R):
        compare(got, gotL, w)
    R.render()                                   # (two marches: the history is kept)
    S = w["nslices"]
    # (mid-frame buffers: 5.2e-4 seen on cfg 3 f32 -- the fp32 error on a steep table ramp before later slices saturate it)
    for k, tol in ((1, TOL), (S // 2, 2 * TOL), (S, TOL)):
        h = R.light_history(k)
        amb = w["lamb_history"][k]
        d = np.abs(h - w["history"][k]).max(axis=2)
        assert d[~amb].max(initial=0) <= tol, f"light_history({k})"


def test_ragged_volume_and_clip_planes(R, O):
    import gl_shadow
    sc = _scene("cfg3", "side", "rot", dims=(40, 24, 18), size=45, shade=1, shadow=(64, 1.0))
    sc.steps, sc.sample_rate = 0, 1.5
    w = gl_shadow.render_shadow(sc)
    push_scene(R, sc)
    for got, gotL in _paths(R):
        compare(got, gotL, w)
    for which in ("orthogonal", "free"):
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
        push_scene(R, sc)
        try:
            for got, gotL in _paths(R):
                compare(got, gotL, w)
        finally:
            sc.clip, sc.clip_plane = None, None
            push_scene(R, sc)


@pytest.mark.parametrize("light,pose", [("oblique", "rot"), ("behind", "back"), ("eye_side", "id")])
def test_depth_equals_the_witness(R, O, light, pose):
    """first-hit depth of the shadowed frame on pixels that are not ambiguous: the view depth of the nearest sample
    with alpha > 0 (+inf where there is none)"""
    import gl_shadow
    sc = _scene("cfg3", light, pose, f32=True, shade=1)
    w = gl_shadow.render_shadow(sc)
    push_scene(R, sc)
    _, d = R.render(depth=True)
    ok = ~w["amb"]
    fin = np.isfinite(w["depth"]) & ok
    assert fin.sum() >= 100
    assert np.array_equal(np.isfinite(d[ok]), np.isfinite(w["depth"][ok]))
    assert np.abs(d[fin] - w["depth"][fin]).max() <= 1e-4


def test_face_coincident_last_slice(R, O):
    """the slice on the far face is drawn in both passes: every pixel and texel matches, no ambiguity allowance"""
    import gl_shadow
    sc = face_scene(O)
    w = gl_shadow.render_shadow(sc)
    push_scene(R, sc)
    for got, gotL in _paths(R):
        compare(got, gotL, w, exact=True)
    R.render()
    S = w["nslices"]
    assert np.abs(R.light_history(S) - w["history"][S]).max() <= TOL
