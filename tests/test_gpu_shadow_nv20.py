"""Half-angle shadows in the NV20 look (option shadow_look 1, smk.h smk_set_shadow): the light buffer's OPACITY attenuates
the eye samples, scaled so that a fully shadowed sample keeps the fraction amb of its colour -- what the reference's fourth
renderer, NV20VolRen3D2, draws on the GeForce3 platform.  The eye pass on the gather kernel, on the slice-ring kernel and
as a launch per slice against the float64 slice pipeline of tests/_nv20_shadow_ref.py under the bounds of
tests/test_shadow_witness.py; the light side against look 0's, bit for bit; the paths among themselves; alpha, depth and
the features that ride along; shards; refusals.  An error of the HIP runtime ends the session."""
import numpy as np
import pytest

import _nv20_shadow_ref as N
from _scenes import push_scene, vgh_volume
from test_shadow_witness import compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def _mode(sc):
    return {0: "none", 1: "r8k" if sc.use_spec else "r8k_diff", 2: "nv20" if sc.use_spec else "nv20_diff"}[sc.shade_mode]


def _push(r, sc, look=1, upload=True):
    """push_scene, then what it leaves at its defaults: gluvv.light.amb and the look"""
    push_scene(r, sc, upload=upload)
    r.set_shading(_mode(sc), sc.light_pos, sc.eye, sc.at, sc.xform, sc.intens, getattr(sc, "amb", N.AMB_DEFAULT))
    r.set_option("shadow_look", look)


def _render(r, smk, **kw):
    """a frame; an error of the HIP runtime ends the session -- nothing more is started on a GPU that has faulted"""
    try:
        return r.render(**kw)
    except smk.SmkError as e:
        if " failed: " in str(e):
            pytest.exit("HIP runtime error, the session ends here: " + str(e), returncode=3)
        raise


def _paths(r, smk, **kw):
    """[(frame or (frame, depth), light buffer)] for kernel 1, kernel 2 and a launch per slice"""
    out = []
    try:
        for kern in (1, 2):
            r.set_option("kernel", kern)
            out.append((_render(r, smk, **kw), r.light_buffer()))
            assert r.last_frame_info()[0] == kern
        r.set_option("kernel", 0)
        r.set_option("shadow_march", 0)
        out.append((_render(r, smk, **kw), r.light_buffer()))
        assert r.last_frame_info()[0] == 3
    finally:
        r.set_option("shadow_march", 1)
        r.set_option("kernel", 0)
    return out


def _paths_agree(r, out, depth=False):
    """gather and slice-ring bit for bit; the per-slice form bit for bit where the slices run away from the viewer, within
    the re-association of the blend (2e-5, tests/test_gpu_shadow.py::test_two_marches_equal_a_launch_per_slice) otherwise"""
    fr = [o[0][0] if depth else o[0] for o in out]
    assert np.array_equal(fr[0], fr[1]), "gather vs slice-ring"
    assert np.array_equal(out[0][1], out[2][1]) and np.array_equal(out[1][1], out[2][1]), "light buffers"
    if r.shadowcoef().front_to_back:
        assert np.array_equal(fr[1], fr[2]), "two marches vs a launch per slice"
    else:
        assert np.abs(fr[1] - fr[2]).max() <= 2e-5
    if depth:
        assert np.array_equal(out[0][0][1], out[1][0][1]) and np.array_equal(out[0][0][1], out[2][0][1]), "depth"


# ---- 1. parity, and 3. the three paths among themselves

@pytest.mark.parametrize("name", sorted(N.CASES))
def test_every_path_equals_the_reference(R, O, smk, name):
    sc, w = N.witness(name)
    _push(R, sc)
    out = _paths(R, smk)
    for k, (got, gotL) in enumerate(out):
        d = np.abs(got - w["rgba"]).max(axis=2)
        print(f"{name} path {k}: unambiguous max {d[~w['amb']].max(initial=0):.3g}, ambiguous pixels {int(w['amb'].sum())}")
        compare(got, gotL, w)
    _paths_agree(R, out)


# ---- 2. the light side is look 0's

@pytest.mark.parametrize("name", ["cfg3-f32-none-eye_side-id-amb0", "tf3d-u8-none-side-back-amb0", "ragged-light-f32-none-oblique-rot-amb.05"])
def test_light_buffer_and_history_equal_look_0(R, O, smk, name):
    sc = N.case_scene(name)
    S = sc.shadowcoef().nslices
    got = {}
    for look in (0, 1):
        _push(R, sc, look=look)
        _render(R, smk)
        got[look] = [R.light_buffer()] + [R.light_history(k) for k in (1, S // 2, S)]
    R.set_option("shadow_look", 0)
    assert got[0][0][..., 3].max() > 0.05
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)


# ---- 4. alpha and depth

def test_unshaded_alpha_and_depth_equal_look_0(R, O, smk):
    sc = N.case_scene("cfg3-u8-none-perp_front-rot-amb.05")
    got = {}
    for look in (0, 1):
        _push(R, sc, look=look)
        got[look] = _paths(R, smk, depth=True)
    R.set_option("shadow_look", 0)
    for (f0, d0), _ in got[0]:
        assert np.isfinite(d0).mean() >= 0.1
    for ((f0, d0), _), ((f1, d1), _) in zip(got[0], got[1]):
        assert np.array_equal(f0[..., 3], f1[..., 3]) and np.array_equal(d0, d1)
        assert np.abs(f0[..., :3] - f1[..., :3]).max() > 1e-2       # (and the colour is another look's)


@pytest.mark.parametrize("name", ["cfg3-u8-dspec-oblique-rot-amb.05", "tf3d-f32-dspec-oblique-id-amb.5"])
def test_phong_amb_scales_colour_never_alpha_or_depth(R, O, smk, name):
    """every operation between f = 1 - sat(La) (1 - amb) and the pixel is monotone in fp32 (a product with a non-negative
    factor, an fma with a non-negative weight), so RGB is non-decreasing in amb exactly; at amb = 1, f = 1 and the sample is
    the unshadowed NV20 sample"""
    outs = []
    for amb in (0.05, 0.5, 1.0):
        _push(R, N.case_scene(name, amb=amb), upload=amb == 0.05)
        outs.append(_paths(R, smk, depth=True))
    R.set_option("shadow_look", 0)
    for path in range(3):
        frames = [o[path][0] for o in outs]
        for (fa, da), (fb, db) in zip(frames, frames[1:]):
            assert np.array_equal(fa[..., 3], fb[..., 3]) and np.array_equal(da, db)
            assert (fb[..., :3] >= fa[..., :3]).all()
        assert np.abs(frames[2][0][..., :3] - frames[0][0][..., :3]).max() > 1e-2


# ---- 5. depth against the reference

@pytest.mark.parametrize("name", ["cfg3-f32-dspec-behind-back-amb.5", "cfg3-u8-dspec-oblique-rot-amb.05", "cfg3-f32-none-eye_side-id-amb0"])
def test_depth_equals_the_reference(R, O, smk, name):
    sc, w = N.witness(name)
    _push(R, sc)
    _, d = _render(R, smk, depth=True)
    ok = ~w["amb"]
    fin = np.isfinite(w["depth"]) & ok
    assert fin.sum() >= 100
    assert np.array_equal(np.isfinite(d[ok]), np.isfinite(w["depth"][ok]))
    assert np.abs(d[fin] - w["depth"][fin]).max() <= 1e-4


# ---- 6. the features that ride along

def _clip_scene(which):
    sc = N.nv20_scene("cfg3", "oblique", "rot", f32=True, shade=2, shadow=(96, 0.7))
    if which == "orthogonal":
        sc.clip = (3, tuple(0.55 * float(f) for f in sc.fsize))
    else:
        n = np.array([0.35, -0.2, -0.9])
        n /= np.linalg.norm(n)
        mv = np.array(sc.mv(), np.float64).reshape(4, 4).T
        centre = mv @ np.array([float(sc.fsize[0]) / 2, float(sc.fsize[1]) / 2, float(sc.fsize[2]) / 2, 1.0])
        sc.clip_plane = (n[0], n[1], n[2], -float(n @ centre[:3]) + 0.03)
    return sc


@pytest.mark.parametrize("which", ["orthogonal", "free"])
def test_clip_planes(R, O, smk, which):
    sc, w = N.witness_of(("clip", which), lambda: _clip_scene(which))
    _push(R, sc)
    try:
        out = _paths(R, smk)
        for got, gotL in out:
            compare(got, gotL, w)
        _paths_agree(R, out)
    finally:
        R.set_clip(0, None)
        R.set_clip_plane(None)


def test_sub_box(R, O, smk):
    sc = N.case_scene("cfg3-u8-dspec-oblique-rot-amb.05")
    _push(R, sc)
    whole = _render(R, smk)
    f = [float(v) for v in sc.fsize]
    R.set_region([6 / 32 * f[0], 0, 0], [f[0], 25 / 32 * f[1], f[2]])
    try:
        out = _paths(R, smk, depth=True)
        _paths_agree(R, out, depth=True)
        assert out[0][0][0][..., 3].max() > 0.05 and np.abs(out[0][0][0] - whole).max() > 1e-2
    finally:
        R.set_region(None)
    assert np.array_equal(_render(R, smk), whole)


def test_time_step_switch_equals_a_fresh_context(gpu_renderer_factory, O, smk):
    scs = []
    for seed in (1, 2):
        sc = N.case_scene("cfg3-f32-dspec-behind-back-amb.5")
        sc.data, sc.grad = vgh_volume(32, seed)[1], vgh_volume(32, seed)[2]
        scs.append(sc)
    fresh = []
    for sc in scs:
        F = gpu_renderer_factory()
        try:
            _push(F, sc)
            fresh.append(_paths(F, smk))
        finally:
            F.close()
    assert not np.array_equal(fresh[0][0][0], fresh[1][0][0])
    r = gpu_renderer_factory()
    try:
        r.set_timestep_cache(2)
        _push(r, scs[0])
        r.upload_timestep(1, scs[1].data, scs[1].grad, fsize=tuple(float(f) for f in scs[1].fsize), dmode="VGH")
        for t in (1, 0):
            r.select_timestep(t)
            for (got, gotL), (want, wantL) in zip(_paths(r, smk), fresh[t]):
                assert np.array_equal(got, want) and np.array_equal(gotL, wantL)
    finally:
        r.close()


def test_scene_depth_goes_to_the_gather_kernel(R, O, smk):
    """no slice-ring instances for scene depth under look 1: auto mode lands on the gather kernel, kernel 2 forced fails with
    the dispatch's reason; the frame is the per-slice form's, and a sample exists only in front of the occluder"""
    sc = N.case_scene("cfg3-u8-dspec-oblique-rot-amb.05")          # (slices away from the viewer: the paths agree bit for bit)
    _push(R, sc)
    assert R.shadowcoef().front_to_back
    plain, d = _render(R, smk, depth=True)
    zs = np.full(d.shape, np.inf, np.float32)
    zs[:, : d.shape[1] // 2] = np.nanmedian(np.where(np.isfinite(d), d, np.nan))
    got, gd = _render(R, smk, depth=True, scene_depth=zs)
    assert R.last_frame_info()[0] == 1
    assert (gd[np.isfinite(gd)] < zs[np.isfinite(gd)]).all()
    assert np.abs(got - plain).max() > 1e-2 and np.array_equal(got[:, d.shape[1] // 2:], plain[:, d.shape[1] // 2:])
    try:
        R.set_option("kernel", 2)
        with pytest.raises(smk.SmkError, match="not applicable: option shadow_look 1 has no scene-depth instances"):
            R.render(scene_depth=zs)
        R.set_option("kernel", 0)
        R.set_option("shadow_march", 0)
        per_slice, pd = _render(R, smk, depth=True, scene_depth=zs)
        assert R.last_frame_info()[0] == 3
        assert np.array_equal(per_slice, got) and np.array_equal(pd, gd)
    finally:
        R.set_option("shadow_march", 1)
        R.set_option("kernel", 0)


@pytest.mark.parametrize("name", ["cfg3-f32-dspec-behind-back-amb.5", "tf3d-u8-none-side-back-amb0"])
def test_brick_flags_on_and_off(R, O, smk, name):
    sc = N.case_scene(name)
    _push(R, sc)
    try:
        on = _paths(R, smk)
        R.set_option("bricks", 0)
        off = _paths(R, smk)
    finally:
        R.set_option("bricks", 1)
    for (a, la), (b, lb) in zip(on, off):
        assert np.array_equal(a, b) and np.array_equal(la, lb)


def test_float_voxels_with_brick_flags_take_a_shape_that_has_an_instance(R, O, smk):
    """the float-voxel 10+2-wave instances with brick flags would spill and are not built: the shape choice passes the
    40x16 and 16x40 pixel tiles over, one forced with option tile is declined with the reason, and without brick flags the
    same tile renders the same frame"""
    sc = N.case_scene("cfg3-f32-dspec-behind-back-amb.5")
    _push(R, sc)
    try:
        R.set_option("kernel", 2)
        want = _render(R, smk)
        assert R.last_frame_info()[0] == 2 and R.stat("slab_plan_bricks") == 1
        assert (R.stat("slab_plan_nw"), R.stat("slab_plan_nl")) != (10, 2)
        R.set_option("tile", 20)
        with pytest.raises(smk.SmkError, match="not applicable: option shadow_look 1 has no float-voxel 10\\+2-wave instances"):
            R.render()
        R.set_option("bricks", 0)
        got = _render(R, smk)
        assert (R.stat("slab_plan_nw"), R.stat("slab_plan_nl")) == (10, 2)
        assert np.array_equal(got, want)
    finally:
        R.set_option("bricks", 1)
        R.set_option("tile", 0)
        R.set_option("kernel", 0)


# ---- 7. shards

def test_two_shards_merge_to_the_unsharded_frame(gpu_renderer_factory, O, smk):
    from simian_spacemonkey_amd import sortlast
    sc = N.case_scene("cfg3-u8-dspec-oblique-rot-amb.05", shadow=(64, 0.75))
    W = gpu_renderer_factory()
    rs = []
    try:
        _push(W, sc)
        ref = _render(W, smk)
        assert ref[..., 3].max() > 0.05 and W.light_buffer()[..., 3].max() > 0.05
        for rank in range(2):
            r = gpu_renderer_factory()
            rs.append(r)
            r.set_shard(rank, 2)
            _push(r, sc)
            need = r.shadow_margin()[1]
            r.close()
            rs[rank] = r = gpu_renderer_factory()
            r.set_shard(rank, 2)
            r.set_option("halo", need)
            _push(r, sc)
        try:
            got = sortlast.render_shadow_frame_local(rs).cpu().numpy()
        except smk.SmkError as e:
            if " failed: " in str(e):
                pytest.exit("HIP runtime error, the session ends here: " + str(e), returncode=3)
            raise
        err = float(np.abs(got - ref).max())
        assert err <= 2e-5, err                  # (tests/test_gpu_shadow_shards.py's TOL)
        _push(W, sc, look=0)                     # (and it is not the R8k frame: NV20 shading has none)
        with pytest.raises(smk.SmkError, match="NV20"):
            W.render()
    finally:
        W.close()
        for r in rs:
            r.close()


# ---- 8. refusals

def test_refusals_and_the_way_back(gpu_renderer_factory, O, smk):
    import oracle
    r = gpu_renderer_factory()
    try:
        base = N.case_scene("cfg3-u8-none-perp_front-rot-amb.05")
        _push(r, base, look=0)
        before = _render(r, smk)
        with pytest.raises(smk.SmkError, match="shadow_look must be 0"):
            r.set_option("shadow_look", 2)
        # look 0 with NV20 shading: today's message
        nv = N.case_scene("cfg3-u8-dspec-oblique-rot-amb.05")
        _push(r, nv, look=0, upload=False)
        with pytest.raises(smk.SmkError, match="NV20 combiners: no shadow mode in NV20VolRen3D"):
            r.render()
        # look 1 with R8k shading
        r8k = N.nv20_scene("cfg3", "oblique", "rot", shade=1)
        _push(r, r8k, upload=False)
        with pytest.raises(smk.SmkError, match="shadow_look 1 is NV20VolRen3D2's: shading none or NV20"):
            r.render()
        # look 1 with perturbation, with and without the R8k look's opt-in
        _push(r, nv, upload=False)
        r.set_perturb(oracle.noise_tex(32), (.2, .1, 0, 0), (.2, 2.1, 4.5, 8.7))
        for opt in (0, 1):
            r.set_option("shadow_perturb", opt)
            with pytest.raises(smk.SmkError, match="shadow_look 1 has no perturbed instances"):
                r.render()
        r.set_option("shadow_perturb", 0)
        r.set_perturb(None, None, None)
        # look 1 with all slices in one cooperative launch, and with the column-stream kernel
        r.set_option("shadow_fused", 1)
        with pytest.raises(smk.SmkError, match="shadow_look 1 has no shadow_fused instances"):
            r.render()
        r.set_option("shadow_fused", 0)
        r.set_option("kernel", 3)
        with pytest.raises(smk.SmkError, match="shadow_look 1: the column-stream kernel has no shadow mode"):
            r.render()
        r.set_option("kernel", 0)
        # the ambient term: finite and in [0, 1] under look 1, unchecked and unused under look 0
        for amb in (1.5, float("nan")):
            bad = N.case_scene("cfg3-u8-none-perp_front-rot-amb.05", amb=amb)
            _push(r, bad, upload=False)
            with pytest.raises(smk.SmkError, match=r"shadow_look 1 needs the ambient term.*\[0, 1\]"):
                r.render()
            _push(r, bad, look=0, upload=False)
            assert np.array_equal(_render(r, smk), before)
        # look 1 with the 1-D table
        one = N.nv20_scene("cfg1", "oblique", "rot")
        _push(r, one)
        with pytest.raises(smk.SmkError, match="shadow_look 1 needs a 2-D or 3-D transfer function"):
            r.render()
        # ... and back: the R8k frame of the context that has been through all of it
        _push(r, base, look=1)
        assert np.abs(_render(r, smk) - before).max() > 1e-2
        _push(r, base, look=0, upload=False)
        assert np.array_equal(_render(r, smk), before)
    finally:
        r.close()
