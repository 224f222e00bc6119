"""Every voxel layout on the three ray-marchers and the slice quad (cases and helpers: tests/_layouts.py, qualified on the
CPU by tests/test_layouts_cpu.py).  nelts 1..4 x u8 / f32, the fourth channel as the second coordinate of the third-axis
table, four-channel f32 with its separate normals buffer (refused by the two streaming kernels, rendered by the gather
kernel), the 13 data modes against the reference's switch, volumes without normals, bricked and shuffled uploads of odd
sizes on whole and sharded contexts, time steps, shadows, f32 values outside [0, 1], and smk_render_slice[_device] called
directly against the float64 quad of oracle/gl_slices.py.

Bounds are the suite's: 1e-4 against the checker (test_gpu_parity.py), slice ring == gather bit for bit (test_gpu_slab.py),
column stream within 2e-5 of gather (test_gpu_cols.py), frames and light buffers with shadows 1e-4 (test_gpu_shadow.py),
the slice quad 1e-4 off its outline with the outline under a tenth of the rest (test_host_adapter.py).  The largest error
of each group is recorded (SMK_LAYOUTS_REPORT=file writes the tally as JSON), not asserted beyond those bounds."""
import ctypes
import json
import os

import numpy as np
import pytest

import _layouts as L

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_G = 2e-5
KERNEL_ID = {1: 1, 2: 2, 3: 4}        # option "kernel" -> smk_last_frame_info's id: gather, slice ring, column stream
F32_4 = "4-channel f32 voxels"
WORST = {}


def _note(group, err):
    WORST[group] = max(WORST.get(group, 0.0), float(err))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlargest error against the checker by group: " + json.dumps(WORST, sort_keys=True))
    if os.environ.get("SMK_LAYOUTS_REPORT"):
        with open(os.environ["SMK_LAYOUTS_REPORT"], "w") as f:
            json.dump(WORST, f, sort_keys=True)


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def _frames(R, kernels=(1, 2, 3)):
    """the current frame set-up under each forced kernel (a forced kernel raises when it does not apply)"""
    out = {}
    try:
        for k in kernels:
            R.set_option("kernel", k)
            out[k] = R.render()
            assert R.last_frame_info()[0] == KERNEL_ID[k]
            assert R.stat("slab_failures") == 0
    finally:
        R.set_option("kernel", 0)
    return out


def _hold(out, ref, group):
    """every kernel's frame against the checker, the streaming kernels against the gather kernel"""
    assert ref[..., 3].max() > 0.05, "scene renders nothing: test is vacuous"
    for k, f in out.items():
        e = np.abs(f - ref).max()
        _note(group, e)
        assert e <= TOL, "kernel %d: max abs err %g" % (k, e)
    if 1 in out and 2 in out:
        assert np.array_equal(out[1], out[2]), "slice ring and gather differ: %g" % np.abs(out[1] - out[2]).max()
    if 1 in out and 3 in out:
        assert np.abs(out[1] - out[3]).max() <= TOL_G, "column stream and gather differ: %g" % np.abs(out[1] - out[3]).max()


def _refused(R, smk, kernel, why):
    R.set_option("kernel", kernel)
    try:
        with pytest.raises(smk.SmkError) as e:
            R.render()
        assert why in str(e.value), str(e.value)
    finally:
        R.set_option("kernel", 0)


# ------------------------------------------------------------------------------------------------ a. channels x type x kernel

CASES = L.channel_cases()


@pytest.mark.parametrize("c", CASES, ids=L.case_id)
def test_channels_types_kernels(R, smk, c):
    sc = L.case_scene(c)
    ref = sc.render()
    L.push(R, sc)
    if sc.nelts == 4 and sc.data.dtype == np.float32:
        # the layout with the separate normals buffer: the streaming kernels say why they do not take it, the automatic
        # choice falls back to the gather kernel
        _refused(R, smk, 2, F32_4)
        _refused(R, smk, 3, F32_4)
        auto = R.render()
        assert R.last_frame_info()[0] == 1 and R.stat("slab_failures") == 0
        out = _frames(R, (1,))
        assert np.array_equal(auto, out[1])
        _hold(out, ref, "a")
    else:
        _hold(_frames(R), ref, "a")


# option "tile" -> the slice-ring kernel's workgroup shape (tests/_slab_plan_cases.py TILES): the big shape fetches its
# voxels early, the small ones late, and each has its own nelts == 4 branch (smk_slab.hip)
SLAB_TILES = {4: (32, 24), 5: (32, 16)}


@pytest.mark.parametrize("tile", sorted(SLAB_TILES))
def test_four_channels_on_both_slice_ring_shapes(R, tile):
    sc = L.scene(4, False, "2d3", shade=1, view="x+", window=L.WINDOWS[0], steps=64)
    L.push(R, sc)
    R.set_option("tile", tile)
    try:
        out = _frames(R, (1, 2))
        assert (R.stat("slab_plan_tw"), R.stat("slab_plan_th")) == SLAB_TILES[tile]
    finally:
        R.set_option("tile", 0)
    _hold(out, sc.render(), "a")


@pytest.mark.parametrize("kernel", [1, 2, 3])
@pytest.mark.parametrize("c", [c for c in CASES if c[0] == 4 and not c[1]], ids=L.case_id)
def test_four_channels_on_two_shards(gpu_renderer_factory, smk, c, kernel):
    """both ranks of a two-rank shard, merged as tests/test_gpu_sortlast.py merges them"""
    import torch
    from simian_spacemonkey_amd import sortlast
    sc = L.case_scene(c)
    ref = sc.render()
    world, npix = 2, sc.width * sc.height
    layers = torch.zeros((world, npix, 4), dtype=torch.float32, device="cuda")
    rs = []
    try:
        for r in range(world):
            Rr = gpu_renderer_factory()
            rs.append(Rr)
            Rr.set_shard(r, world)
            L.push(Rr, sc)
            Rr.set_option("kernel", kernel)
            Rr.render_device(layers[r].data_ptr(), None, None)
        torch.cuda.synchronize()
        for Rr in rs:
            assert Rr.last_frame_info()[0] == KERNEL_ID[kernel]
            assert Rr.stat("slab_status") == 0 and Rr.stat("slab_failures") == 0
        order = rs[0].shard_order(world)
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        rs[0].composite_over_device(layers.data_ptr(), world, order, npix, out.data_ptr(), None)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(sc.height, sc.width, 4)
        e = np.abs(got - ref).max()
        _note("a", e)
        assert ref[..., 3].max() > 0.05 and e <= TOL
        for r in range(world):
            part = L.case_scene(c)
            part.region = sortlast.shard_region(sc.dims, r, world)
            pr = part.render()
            e = np.abs(layers[r].cpu().numpy().reshape(sc.height, sc.width, 4) - pr).max()
            _note("a", e)
            assert pr[..., 3].max() > 0.05 and e <= TOL, r
    finally:
        for Rr in rs:
            Rr.close()


# ------------------------------------------------------------------------------------------------ b. the data-mode rule

def _without_second_table(R, sc, kernels):
    R.set_tf2d(sc.tf_vg, None)
    try:
        return _frames(R, kernels)
    finally:
        R.set_tf2d(sc.tf_vg, sc.tf_h)


@pytest.mark.parametrize("mode", L.MODES)
@pytest.mark.parametrize("nelts", L.RULE_VOLUMES)
def test_data_mode_rule(R, nelts, mode):
    """a second table is set under every mode; the frame follows the reference's switch (L.THIRD, NV20VolRen3D.cpp:686-693),
    and outside it the second table changes no bit.  One mode of each kind also on the streaming kernels"""
    sc = L.rule_scene(nelts, mode)
    assert sc.tf_h is not None and sc.third_axis == (1 if mode in L.THIRD else 0)
    kernels = (1, 2, 3) if mode in ("V3G", "V2") else (1,)
    L.push(R, sc)
    out = _frames(R, kernels)
    _hold(out, sc.render(), "b")
    none = _without_second_table(R, sc, kernels)
    for k in kernels:
        if sc.third_axis:
            assert np.abs(out[k] - none[k]).max() > 1e-2
        else:
            assert np.array_equal(out[k], none[k]), "kernel %d: the second table shows under %s" % (k, mode)


def test_two_channels_have_no_third_axis(R):
    """VGH with a second table on a two-channel volume: the nelts >= 3 clause"""
    sc = L.rule_scene(2, "VGH")
    assert sc.tf_h is not None and sc.third_axis == 0
    L.push(R, sc)
    out = _frames(R)
    _hold(out, sc.render(), "b")
    none = _without_second_table(R, sc, (1, 2, 3))
    for k in out:
        assert np.array_equal(out[k], none[k])


# ------------------------------------------------------------------------------------------------ c. no normals

@pytest.mark.parametrize("f32", [False, True])
def test_shading_requested_without_normals(R, f32):
    sc = L.no_normals_scene(f32)
    assert sc.grad is None and sc.shade_mode == 1
    L.push(R, sc)
    _hold(_frames(R), sc.render(), "c")       # (the checker's frame of this scene is the unshaded one: test_layouts_cpu.py)


# ------------------------------------------------------------------------------------------------ d. packing

def _pack_kernel(nelts, f32, world):
    if f32:
        return 1 if nelts == 4 else 3 if world == 1 else 1
    return 2


@pytest.mark.parametrize("rank,world", L.PACK_SHARDS)
@pytest.mark.parametrize("nelts,f32", L.PACK_LAYOUTS)
def test_bricked_and_shuffled_uploads(gpu_renderer_factory, smk, nelts, f32, rank, world):
    from simian_spacemonkey_amd import sortlast
    sc = L.pack_scene(nelts, f32)
    if world > 1:
        sc.region = sortlast.shard_region(sc.dims, rank, world)
    ref = sc.render()
    k = _pack_kernel(nelts, f32, world)
    Rr = gpu_renderer_factory()
    try:
        if world > 1:
            Rr.set_shard(rank, world)
        L.push(Rr, sc)
        whole = _frames(Rr, (k,))
        _hold(whole, ref, "d")
        for grid in L.PACK_GRIDS:
            n = grid[0] * grid[1] * grid[2]
            L.push(Rr, sc, grid, L.shuffled(n))
            got = _frames(Rr, (k,))
            assert np.array_equal(got[k], whole[k]), "bricks %s: %g" % (grid, np.abs(got[k] - whole[k]).max())
    finally:
        Rr.close()


@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_upload_from_device_memory(gpu_renderer_factory, rank, world):
    """smk_upload_volume_device of the bricked four-channel f32 volume with normals: the bits of the host upload"""
    import torch
    from simian_spacemonkey_amd import sortlast
    sc = L.pack_scene(4, True)
    if world > 1:
        sc.region = sortlast.shard_region(sc.dims, rank, world)
    ref = sc.render()

    def dev(a):
        t = torch.from_numpy(np.array(a)).cuda()       # (the cases' arrays are read-only)
        return t.data_ptr(), t
    Rr = gpu_renderer_factory()
    try:
        if world > 1:
            Rr.set_shard(rank, world)
        L.push(Rr, sc, (3, 1, 2), L.shuffled(6))
        host = _frames(Rr, (1,))
        keep = L.upload(Rr, sc, (3, 1, 2), L.shuffled(6), to_device=dev, ready=torch.cuda.synchronize)
        torch.cuda.synchronize()
        got = _frames(Rr, (1,))
        del keep
        assert np.array_equal(got[1], host[1])
        _hold(got, ref, "d")
    finally:
        Rr.close()


# ------------------------------------------------------------------------------------------------ e. time steps

def test_time_steps_switch_the_normals_buffer(gpu_renderer_factory):
    import torch
    scs = L.step_scenes()
    refs = [s.render() for s in scs]
    assert np.abs(refs[0] - refs[1]).max() > 1e-2
    st = torch.cuda.Stream()

    def dev(a):
        t = torch.from_numpy(np.array(a)).cuda()       # (the cases' arrays are read-only)
        return t.data_ptr(), t
    Rr = gpu_renderer_factory()
    try:
        Rr.set_timestep_cache(2)
        L.push(Rr, scs[0])
        keep = L.upload(Rr, scs[1], to_device=dev, timestep=1, stream=ctypes.c_void_p(st.cuda_stream),
                        ready=torch.cuda.synchronize)       # (the caller's stream does not wait for the copies by itself)
        st.synchronize()
        del keep
        assert Rr.timesteps() == (0, [0, 1])
        frames = []
        for t in (0, 1, 0, 1):
            Rr.select_timestep(t)
            f = Rr.render()
            assert Rr.last_frame_info()[0] == 1          # (four-channel f32: the gather kernel)
            e = np.abs(f - refs[t]).max()
            _note("e", e)
            assert e <= TOL, (t, e)
            frames.append(f)
        assert np.array_equal(frames[0], frames[2]) and np.array_equal(frames[1], frames[3])
        assert np.abs(frames[0] - frames[1]).max() > 1e-2
    finally:
        Rr.close()


# ------------------------------------------------------------------------------------------------ f. shadows

def _shadow_fields(a):
    return {f: (list(getattr(a, f)) if hasattr(getattr(a, f), "__len__") else getattr(a, f)) for f, _ in a._fields_}


# every path the existing shadow tests force: the two marches under the automatic choice and under each ray-marcher, a
# launch per slice (smk_shadow.hip), all slices in one cooperative launch
SHADOW_PATHS = {"auto": {}, "gather": {"kernel": 1}, "slice_ring": {"kernel": 2}, "per_slice": {"shadow_march": 0},
                "fused": {"shadow_fused": 1}}
RESET = {"kernel": 0, "shadow_march": 1, "shadow_fused": 0}


@pytest.mark.parametrize("f32,path", [(False, p) for p in SHADOW_PATHS] + [(True, "auto"), (True, "gather")])
def test_shadows_with_four_channels(R, f32, path):
    """light, buffer and quality as the existing small shadow tests have them (_layouts.SHADOW, SHADOW_LIGHT); the pair
    passes the checker's own light-buffer qualification (test_layouts_cpu.py), none had to be replaced"""
    sc = L.shadow_scene(f32)
    ref, refL = sc.render_shadow()
    assert ref[..., 3].max() > 0.05 and refL[..., 3].max() > 0.05, "vacuous scene"
    L.push(R, sc)
    try:
        assert _shadow_fields(R.shadowcoef()) == _shadow_fields(sc.shadowcoef())
        for k, v in SHADOW_PATHS[path].items():
            R.set_option(k, v)
        got = R.render()
        gotL = R.light_buffer()
        want_id = {"auto": (1,) if f32 else (1, 2), "gather": (1,), "slice_ring": (2,), "per_slice": (3,), "fused": (3,)}[path]
        assert R.last_frame_info()[0] in want_id
        assert R.stat("slab_failures") == 0
    finally:
        for k, v in RESET.items():
            R.set_option(k, v)
        R.set_shadow(0)
    assert gotL.shape == refL.shape
    eL, e = np.abs(gotL - refL).max(), np.abs(got - ref).max()
    _note("f", e)
    _note("f_light", eL)
    assert eL <= TOL, "light buffer max abs err %g" % eL
    assert e <= TOL, "frame max abs err %g" % e


# ------------------------------------------------------------------------------------------------ g. f32 outside [0, 1]

def test_f32_values_outside_the_unit_range(R):
    sc = L.wide_range_scene()
    ref = sc.render()
    try:
        L.push(R, sc)
        R.set_option("bricks", 1)
        on = _frames(R)
        _hold(on, ref, "g")
        R.set_option("bricks", 0)
        off = _frames(R)
        for k in on:
            assert np.array_equal(on[k], off[k]), "kernel %d: the brick flags changed the frame" % k
    finally:
        R.set_option("bricks", 1)


# ------------------------------------------------------------------------------------------------ h. the slice quad

_SLICE_REF = {}


def _slice_ref(f32, window, name, alpha, seed=3):
    """(base frame, reference frame, edge mask), shared by the volumes of one type: the quad shows channel 0, which they
    share, over the checker's frame of the one-channel volume"""
    key = (f32, window, name, alpha, seed)
    if key not in _SLICE_REF:
        bkey = (f32, window, seed)
        if bkey not in _SLICE_REF:
            _SLICE_REF[bkey] = L.slice_scene(1, f32, window, seed).render()
        base = _SLICE_REF[bkey]
        sc = L.slice_scene(1, f32, window, seed)
        want, edge = L.slice_reference(sc, base, L.quads(sc)[name], alpha)
        _SLICE_REF[key] = (base, want, edge)
    return _SLICE_REF[key]


def _check_slice(got, f32, window, name, alpha, seed=3):
    base, want, edge = _slice_ref(f32, window, name, alpha, seed)
    inner = ~edge
    assert base[..., 3].max() > 0.05
    assert edge.sum() < 0.1 * inner.sum()
    if name in L.NO_DRAW:
        assert np.array_equal(got, base), "%s quad at alpha %g: %d pixels touched" % (name, alpha, (got != base).any(-1).sum())
    else:
        assert np.abs(want - base).max() > 0.05
        e = np.abs(got[inner] - want[inner]).max()
        _note("h", e)
        assert e <= 1e-4, "%s quad at alpha %g: %g" % (name, alpha, e)


@pytest.mark.parametrize("window", sorted({w for w, _ in L.SLICE_CASES}), ids=lambda w: "%dx%d" % w)
@pytest.mark.parametrize("nelts", [1, 3, 4])
@pytest.mark.parametrize("f32", [False, True])
def test_slice_quad(R, f32, nelts, window):
    sc = L.slice_scene(nelts, f32, window)
    L.push(R, sc)
    quads = L.quads(sc)
    for w, name in L.SLICE_CASES:
        if w != window:
            continue
        for alpha in L.ALPHAS:
            base = _slice_ref(f32, window, name, alpha)[0]
            got = R.render_slice(quads[name], alpha, base.copy())
            _check_slice(got, f32, window, name, alpha)


@pytest.mark.parametrize("f32", [False, True])
def test_slice_quad_device_entry_on_a_caller_stream(R, f32):
    import torch
    window = (37, 29)
    sc = L.slice_scene(4, f32, window)
    L.push(R, sc)
    st = torch.cuda.Stream()
    for name in ("oblique", "outside", "behind"):
        q = np.ascontiguousarray(L.quads(sc)[name], np.float32).reshape(12)
        base = _slice_ref(f32, window, name, 0.6)[0]
        host = R.render_slice(L.quads(sc)[name], 0.6, base.copy())
        d = torch.from_numpy(base.copy()).cuda()
        torch.cuda.synchronize()
        R._ck(R.L.smk_render_slice_device(R.ctx, q.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 0.6,
                                          ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(st.cuda_stream)))
        st.synchronize()
        assert np.array_equal(d.cpu().numpy(), host), name
        _check_slice(host, f32, window, name, 0.6)


def test_slice_quad_shows_the_selected_time_step(gpu_renderer_factory):
    window, f32 = (37, 29), True
    scs = [L.slice_scene(3, f32, window, seed=s) for s in (3, 4)]
    Rr = gpu_renderer_factory()
    try:
        Rr.set_timestep_cache(2)
        L.push(Rr, scs[0])
        L.upload(Rr, scs[1], timestep=1)
        q = L.quads(scs[0])["oblique"]
        got = {}
        for t in (1, 0, 1):
            Rr.select_timestep(t)
            base = _slice_ref(f32, window, "oblique", 0.6, seed=3 + t)[0]
            got[t] = Rr.render_slice(q, 0.6, base.copy())
            _check_slice(got[t], f32, window, "oblique", 0.6, seed=3 + t)
        w0, w1 = (_slice_ref(f32, window, "oblique", 0.6, seed=s)[1] for s in (3, 4))
        assert np.abs(w0 - w1).max() > 0.05
    finally:
        Rr.close()


def test_slice_quad_refusals(R, smk, gpu_renderer_factory):
    sc = L.slice_scene(1, False)
    L.push(R, sc)
    q = np.ascontiguousarray(L.quads(sc)["oblique"], np.float32).reshape(12)
    qp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    frame = np.zeros((sc.height, sc.width, 4), np.float32)
    fp = frame.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def refused(r, rc, why):
        assert rc != 0 and why in r.L.smk_last_error(r.ctx).decode(), r.L.smk_last_error(r.ctx).decode()
    refused(R, R.L.smk_render_slice(R.ctx, qp, 0.6, None), "smk_render_slice: null frame")
    refused(R, R.L.smk_render_slice(R.ctx, None, 0.6, fp), "smk_render_slice: null argument")
    refused(R, R.L.smk_render_slice_device(R.ctx, qp, 0.6, None, None), "smk_render_slice: null argument")
    assert not frame.any()
    r2 = gpu_renderer_factory()
    try:
        refused(r2, r2.L.smk_render_slice(r2.ctx, qp, 0.6, fp), "smk_render_slice: no camera set")
        L.frame_state(r2, sc)
        refused(r2, r2.L.smk_render_slice(r2.ctx, qp, 0.6, fp), "smk_render_slice: no volume uploaded")
    finally:
        r2.close()
    r3 = gpu_renderer_factory()
    try:
        L.upload(r3, sc)
        refused(r3, r3.L.smk_render_slice(r3.ctx, qp, 0.6, fp), "smk_render_slice: no camera set")
    finally:
        r3.close()
    r4 = gpu_renderer_factory()
    try:
        r4.set_shard(0, 2)
        L.push(r4, sc)
        with pytest.raises(smk.SmkError, match="drawn from the whole volume"):
            r4.render_slice(L.quads(sc)["oblique"], 0.6, frame)
    finally:
        r4.close()
    assert not frame.any()
