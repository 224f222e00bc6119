"""The clip-plane widget's data slice drawn with the volume frame (smk.h smk_set_clip_slice) against the float64 checker
tests/_clip_slice_ref.py.  V = the frame the SAME context renders without the slice, S = the checker's slice layer:
the frame must be compose(V, S) to the project's parity bound where the reference's rule draws a pass, V bit for bit
where it draws none; the depth test, GL_MAX, shadows, depth_out, time steps and the refusals as the header states them.

Pixels whose centre lies within 1e-3 px of a projected quad edge are left out (an edge decision in other arithmetic); they
must be <= 0.1 % of the covered pixels -- tests/test_clip_slice_ref.py checks on the CPU that the poses used here
(_clip_slice_cases.CASE_POSE) do not hinge on such decisions."""
import numpy as np
import pytest

import _clip_slice_ref as CS
from _clip_slice_cases import AXES, CASE_POSE, PASS_TABLE, SIZE, clip_vpos, widget_corners
from _scenes import make_scene, push_scene, vgh_volume

pytestmark = pytest.mark.gpu
TOL = 1e-4      # the project's parity bound
ZFAR = 20.0     # push_scene's far plane
ALPHA = 0.6
KERNEL_RAN = {1: 0, 2: 0, 3: 0}


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _restore(R):
    yield
    R.set_option("kernel", 0)
    R.set_blend(0)
    R.set_clip_slice(None)


def _scene(oaxis, f32=True, frac=0.45, margin=0.25, **kw):
    sc = make_scene("cfg3", n=32, size=SIZE, steps=48, pose=CASE_POSE[oaxis], f32=f32, shade=1, **kw)
    vpos = clip_vpos(oaxis, sc.fsize, frac)
    sc.clip = (oaxis, vpos)
    return sc, widget_corners(oaxis, vpos, sc.fsize, margin)


def _layer(sc, corners, oaxis, look, alpha=ALPHA, scene_depth=None, data=None):
    return CS.slice_layer(sc.data if data is None else data, "VGH", sc.fsize, sc.mv(), sc.frustum, sc.znear, sc.width,
                          sc.height, corners, oaxis, alpha, look, scene_depth=scene_depth)


def _edges(sc, corners, oaxis, cover):
    edge = CS.edge_pixels(CS.moved_quad(corners, sc.fsize, oaxis), sc.mv(), sc.frustum, sc.znear, ZFAR, sc.width, sc.height)
    assert cover.sum() > 300, "vacuous: the quad covers %d pixels" % cover.sum()
    assert edge.sum() <= 1e-3 * cover.sum(), (edge.sum(), cover.sum())
    return edge


def _check(got, V, S, cover, edge, pass_, blend_max=False, what=""):
    """frame == compose(V, S) within TOL on the covered pixels, == V bit for bit everywhere else"""
    want = CS.compose(V, S, cover, pass_, blend_max)
    keep = ~edge
    err = np.abs(got.astype(np.float64) - want)[keep].max()
    print("%s pass %d: max |frame - compose(V, S)| = %.3g over %d covered pixels" % (what, pass_, err, cover.sum()))
    assert err <= TOL, (what, err)
    assert np.array_equal(got[~cover & keep], V[~cover & keep]), what
    if pass_:
        assert np.abs(got - V)[cover & keep].max() > 1e-3, "vacuous: the slice changes nothing"


def _try_kernel(R, kernel):
    """the frame without the slice on that ray-marcher, or None where it declines the frame (forced kernels 2, 3 do)"""
    R.set_option("kernel", kernel)
    R.set_clip_slice(None)
    try:
        V = R.render()
    except Exception as e:    # SmkError: "... forced but not applicable ..."
        assert kernel != 1 and "not applicable" in str(e), e
        return None
    assert R.last_frame_info()[0] == {1: 1, 2: 2, 3: 4}[kernel]
    KERNEL_RAN[kernel] += 1
    return V


# ---------------------------------------------------------------------------------- 1. every axis, sign, look, dtype

@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("oaxis", sorted(AXES))
def test_slice_composes_with_the_volume_frame(R, oaxis, f32):
    sc, corners = _scene(oaxis, f32)
    push_scene(R, sc)
    layers = {look: _layer(sc, corners, oaxis, look) for look in ("r8k", "nv20")}
    edge = _edges(sc, corners, oaxis, layers["r8k"][1])
    for kernel in (1, 2, 3):
        V = _try_kernel(R, kernel)
        if V is None:
            continue
        assert V[..., 3].max() > 0.05, "vacuous volume frame"
        for dv, want_pass in ((-0.5, PASS_TABLE[oaxis][0]), (0.5, PASS_TABLE[oaxis][1])):
            assert CS.pass_rule(oaxis, dv, corners, sc.fsize) == want_pass
            for look, (S, cover, _) in layers.items():
                R.set_clip_slice(corners, ALPHA, dv, look)
                got = R.render()
                assert R.stat("clip_slice_pass") == want_pass
                _check(got, V, S, cover, edge, want_pass, what="%s dv %+g %s kernel %d f32 %d" % (AXES[oaxis], dv, look, kernel, f32))
        # dv == 0: neither pass
        R.set_clip_slice(corners, ALPHA, 0.0, "r8k")
        assert np.array_equal(R.render(), V) and R.stat("clip_slice_pass") == 0


def test_the_streaming_kernels_took_part():
    """(runs after the cases above) forced kernels may decline a pose; the slice-ring kernel must have rendered some"""
    assert KERNEL_RAN[1] >= 12 and KERNEL_RAN[2] >= 1, KERNEL_RAN


@pytest.mark.parametrize("oaxis", sorted(AXES))
def test_plane_outside_the_volume(R, oaxis):
    """corner 0 not strictly inside (0, fSize): no pass, the frame is V bit for bit -- except on X-, which the reference
    draws without that test (R8kVolRen3D.cpp:835)"""
    sc, corners = _scene(oaxis, frac=1.3)
    push_scene(R, sc)
    R.set_option("kernel", 1)
    V = R.render()
    for dv in (-0.5, 0.5):
        R.set_clip_slice(corners, ALPHA, dv, "r8k")
        got = R.render()
        want_pass = CS.pass_rule(oaxis, dv, corners, sc.fsize)
        assert R.stat("clip_slice_pass") == want_pass
        if oaxis != 2:
            assert want_pass == 0 and np.array_equal(got, V)
        else:
            assert want_pass == (1 if dv > 0 else 2)
            S, cover, _ = _layer(sc, corners, oaxis, "r8k")
            edge = CS.edge_pixels(CS.moved_quad(corners, sc.fsize, oaxis), sc.mv(), sc.frustum, sc.znear, ZFAR, SIZE, SIZE)
            assert cover.sum() > 300 and edge.sum() <= 1e-3 * cover.sum()
            _check(got, V, S, cover, edge, want_pass, what="X- outside")


def test_a_quad_inside_the_cut_face(R):
    """a rectangle smaller than the volume's face: its own edges bound the slice"""
    oaxis = 5
    sc, corners = _scene(oaxis, f32=False, margin=-0.2)
    push_scene(R, sc)
    R.set_option("kernel", 1)
    V = R.render()
    S, cover, _ = _layer(sc, corners, oaxis, "r8k")
    edge = _edges(sc, corners, oaxis, cover)
    for dv in (-0.5, 0.5):
        R.set_clip_slice(corners, ALPHA, dv, "r8k")
        _check(R.render(), V, S, cover, edge, CS.pass_rule(oaxis, dv, corners, sc.fsize), what="inner quad dv %+g" % dv)


# ------------------------------------------------------------------------------------------------ 2. off means off

@pytest.mark.parametrize("kernel", [1, 2])
def test_off_is_bit_identical(R, gpu_renderer_factory, kernel):
    """on = 0 after the slice was on, and a context that never made the call: the same bits under every blend, with
    shadows and with a scene depth"""
    oaxis = 1
    sc, corners = _scene(oaxis)
    zs = np.full((SIZE, SIZE), 6.9, np.float32)

    def frames(r):
        out = []
        r.set_option("kernel", kernel)
        r.set_option("slab_split", 1)       # (no measured depth cuts: two contexts' slice-ring frames hold the same bits)
        for blend in (0, 1, 2):
            r.set_blend(blend)
            out.append(r.render())
            out.append(r.render(scene_depth=zs))
        r.set_blend(0)
        return out

    def shadowed(r):
        s2, _ = _scene(oaxis)
        s2.light_pos = (3, 4, 3)
        s2.shadow = (64, 0.7)
        push_scene(r, s2, upload=False)
        r.set_option("kernel", kernel)
        return [r.render(), r.render(scene_depth=zs)]

    fresh = gpu_renderer_factory()
    try:
        push_scene(fresh, sc)
        never = frames(fresh) + shadowed(fresh)
    finally:
        fresh.close()
    push_scene(R, sc)
    R.set_option("kernel", kernel)
    R.set_clip_slice(corners, ALPHA, -0.5, "r8k")
    drawn = R.render()
    assert R.stat("clip_slice_pass") == 1
    R.set_clip_slice(None)
    off = frames(R) + shadowed(R)
    assert R.stat("clip_slice_pass") == 0
    assert not np.array_equal(drawn, off[0])
    for a, b in zip(never, off):
        assert np.array_equal(a, b)
    R.set_shadow(0)
    R.set_option("slab_split", 0)


def test_clip_off_draws_nothing(R):
    sc, corners = _scene(1)
    sc.clip = None
    push_scene(R, sc)
    R.set_option("kernel", 1)
    V = R.render()
    R.set_clip_slice(corners, ALPHA, -0.5, "r8k")
    assert np.array_equal(R.render(), V) and R.stat("clip_slice_pass") == 0
    R.set_clip(1, clip_vpos(1, sc.fsize))
    assert R.render() is not None and R.stat("clip_slice_pass") == 1


# ---------------------------------------------------------------------------------------------------- 3. depth test

def _window_depth(d, n, f):
    return ((f - f * n / np.asarray(d, np.float64)) / (f - n)).astype(np.float32)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("dv", [-0.5, 0.5])
def test_occluder_through_the_middle_of_the_quad(R, dv, kind):
    """a fronto-parallel occluder at the quad's median depth: slice pixels behind it are V, those in front compose(V, S)"""
    oaxis = 1
    sc, corners = _scene(oaxis)
    push_scene(R, sc)
    R.set_option("kernel", 1)
    _, cover0, depth = _layer(sc, corners, oaxis, "r8k")
    d_mid = float(np.median(depth[cover0]))
    n, f = sc.znear, ZFAR
    if kind == 0:
        zs = np.full((SIZE, SIZE), d_mid, np.float32)
        zview = zs
    else:
        zs = np.full((SIZE, SIZE), _window_depth(d_mid, n, f), np.float32)
        zview = (f * n / (f - zs.astype(np.float64) * (f - n))).astype(np.float32)     # smk.h: in double, rounded once
    V = R.render(scene_depth=zs, scene_depth_kind=kind)
    S, cover, _ = _layer(sc, corners, oaxis, "r8k", scene_depth=zview)
    behind = cover0 & ~cover
    assert cover.sum() > 100 and behind.sum() > 100, (cover.sum(), behind.sum())
    edge = _edges(sc, corners, oaxis, cover0)
    R.set_clip_slice(corners, ALPHA, dv, "r8k")
    got = R.render(scene_depth=zs, scene_depth_kind=kind)
    want_pass = CS.pass_rule(oaxis, dv, corners, sc.fsize)
    assert R.stat("clip_slice_pass") == want_pass
    _check(got, V, S, cover, edge, want_pass, what="occluded kind %d dv %+g" % (kind, dv))
    assert np.array_equal(got[behind & ~edge], V[behind & ~edge])


def test_depth_out_is_the_volume_alone(R):
    sc, corners = _scene(3)
    push_scene(R, sc)
    for kernel in (1, 2):
        if _try_kernel(R, kernel) is None:
            continue
        V, d0 = R.render(depth=True)
        for dv in (-0.5, 0.5):
            R.set_clip_slice(corners, ALPHA, dv, "r8k")
            got, d1 = R.render(depth=True)
            assert R.stat("clip_slice_pass") in (1, 2)
            assert not np.array_equal(got, V) and np.array_equal(d0, d1)
        R.set_clip_slice(None)


# --------------------------------------------------------------------------------------------------------- 4. blends

def test_gl_max_before_pass_is_the_maximum(R):
    oaxis = 1
    sc, corners = _scene(oaxis)
    push_scene(R, sc)
    R.set_blend(2)
    S, cover, _ = _layer(sc, corners, oaxis, "nv20")
    edge = _edges(sc, corners, oaxis, cover)
    for kernel in (1, 2):
        V = _try_kernel(R, kernel)
        if V is None:
            continue
        R.set_clip_slice(corners, ALPHA, -0.5, "nv20")
        got = R.render()
        assert R.stat("clip_slice_pass") == 1
        _check(got, V, S, cover, edge, 1, blend_max=True, what="GL_MAX kernel %d" % kernel)
        # the maximum itself is exact: the frame is V or the product's own slice value, component by component
        k = cover & ~edge
        assert np.all((got[k] == V[k]) | (got[k] > V[k]))


def test_both_over_orders_get_the_same_slice_layer(R):
    """where the volume layer is exactly zero the frame IS the slice layer: back-to-front and front-to-back frames hold
    the same bits there"""
    oaxis = 1
    sc, corners = _scene(oaxis)
    push_scene(R, sc)
    R.set_option("kernel", 1)
    frames, vols = [], []
    for blend in (0, 1):
        R.set_blend(blend)
        R.set_clip_slice(None)
        vols.append(R.render())
        R.set_clip_slice(corners, ALPHA, -0.5, "r8k")
        frames.append(R.render())
    _, cover, _ = _layer(sc, corners, oaxis, "r8k")
    bare = cover & np.all(vols[0] == 0, axis=-1) & np.all(vols[1] == 0, axis=-1)
    assert bare.sum() > 50, bare.sum()
    assert np.array_equal(frames[0][bare], frames[1][bare]) and frames[0][bare][:, 3].min() > 0


# -------------------------------------------------------------------------------------------------------- 5. shadows

@pytest.mark.parametrize("light,along", [((3, 4, -3), True), ((3, 4, 3), False)])
def test_shadows(R, light, along):
    """axis X+: dv < 0 says before, dv > 0 after.  A light with vdl > 0 drops the before pass (frame == V, stat 0); the
    after pass is always drawn; the light buffer never sees the slice"""
    oaxis = 1
    sc, corners = _scene(oaxis)
    sc.light_pos = light
    sc.shadow = (64, 0.7)
    push_scene(R, sc)
    R.set_option("kernel", 1)
    assert bool(R.shadowcoef().front_to_back) == along      # vdl > 0 (smk_shadow_plan.hip)
    vdl = 1.0 if along else -1.0
    V = R.render()
    lb0 = R.light_buffer()
    assert V[..., 3].max() > 0.05 and lb0[..., 3].max() > 0
    S, cover, _ = _layer(sc, corners, oaxis, "r8k")
    edge = _edges(sc, corners, oaxis, cover)
    for dv in (-0.5, 0.5):
        want_pass = CS.pass_rule(oaxis, dv, corners, sc.fsize, vdl=vdl)
        assert want_pass == ((0 if along else 1) if dv < 0 else 2)
        R.set_clip_slice(corners, ALPHA, dv, "r8k")
        got = R.render()
        assert R.stat("clip_slice_pass") == want_pass
        if want_pass == 0:
            assert np.array_equal(got, V)
        else:
            _check(got, V, S, cover, edge, want_pass, what="shadows light %s dv %+g" % (light, dv))
        assert np.array_equal(R.light_buffer(), lb0)
    R.set_shadow(0)


# ----------------------------------------------------------------------------------------------------- 6. time steps

def test_the_slice_shows_the_selected_time_step(gpu_renderer_factory):
    oaxis = 5
    sc, corners = _scene(oaxis, f32=False)
    other = vgh_volume(32, 2)
    r = gpu_renderer_factory()
    try:
        r.set_timestep_cache(2)
        push_scene(r, sc)
        r.set_option("kernel", 1)
        r.upload_timestep(1, other[0], other[2], fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
        layers = [_layer(sc, corners, oaxis, "r8k"), _layer(sc, corners, oaxis, "r8k", data=other[0])]
        edge = _edges(sc, corners, oaxis, layers[0][1])
        assert np.abs(layers[0][0] - layers[1][0]).max() > 0.05, "the steps' slices do not differ"
        for t in (1, 0, 1):
            r.select_timestep(t)
            r.set_clip_slice(None)
            V = r.render()
            r.set_clip_slice(corners, ALPHA, 0.5, "r8k")
            _check(r.render(), V, layers[t][0], layers[t][1], edge, 2, what="time step %d" % t)
    finally:
        r.close()


# --------------------------------------------------------------------------------------------------------- 7. refusals

def test_bad_arguments_are_refused_with_the_reason(R, smk):
    sc, corners = _scene(1)
    push_scene(R, sc)
    with pytest.raises(smk.SmkError, match="look"):
        R.set_clip_slice(corners, ALPHA, 0.5, 7)
    bad = corners.copy()
    bad[2, 1] = np.nan
    with pytest.raises(smk.SmkError, match="corner 2 is not finite"):
        R.set_clip_slice(bad, ALPHA, 0.5, "r8k")
    bad[2, 1] = np.inf
    with pytest.raises(smk.SmkError, match="not finite"):
        R.set_clip_slice(bad, ALPHA, 0.5, "r8k")
    with pytest.raises(smk.SmkError, match="dv is not finite"):
        R.set_clip_slice(corners, ALPHA, float("nan"), "r8k")
    with pytest.raises(smk.SmkError, match="alpha is not finite"):
        R.set_clip_slice(corners, float("inf"), 0.5, "r8k")
    # a refused call changes nothing
    R.set_option("kernel", 1)
    V = R.render()
    assert R.stat("clip_slice_pass") == 0 and V[..., 3].max() > 0.05
