"""SMK_U16 voxels on the GPU (include/smk.h; cases and numpy restatements: tests/_u16_ref.py, qualified on the CPU by
tests/test_u16_cpu.py).  The reference is the CPU checker rendering decode_u16(volume) as an f32 volume; the bound is the
project's 1e-4 for every kernel.  The gather kernel renders every mode; the slice-ring kernel has the plain instances and
the eye pass of frames with shadows under look 0, bit-identical to the gather kernel's frames (option slab_split 1: no
measured depth cuts; a back-to-front frame, which it composites front to back, within 2e-5), and declines frames with the
host's scene depth or the NV20 look with the reason; the column-stream kernel refuses the type."""
import ctypes

import numpy as np
import pytest

import _layouts as L
import _u16_ref as U

pytestmark = pytest.mark.gpu
TOL = U.TOL
NO_OCC = "u16 voxels have no scene-depth instances of the slice-ring kernel"
NO_NV20 = "u16 voxels have no shadow_look 1 instances of the slice-ring kernel"
TOL_REASSOC = 2e-5      # against the gather kernel where the blend is re-associated (tests/test_gpu_slab_plans.py)
SLAB_RAN = {}           # view -> frames the slice-ring kernel rendered
NO_COLS = "u16 voxels (the column-stream kernel has no u16 instance)"


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _restore(R):
    yield
    for k, v in (("kernel", 0), ("bricks", 1), ("shadow_march", 1), ("shadow_fused", 0), ("shadow_look", 0), ("slab_split", 0),
                 ("tile", 0)):
        R.set_option(k, v)
    R.set_blend(0)
    R.set_shadow(0)
    R.set_perturb(None, None, None)
    R.set_clip(0, None)
    R.set_clip_slice(None)


def _gather(R, **kw):
    R.set_option("kernel", 1)
    try:
        out = R.render(**kw)
        assert R.last_frame_info()[0] == 1
    finally:
        R.set_option("kernel", 0)
    return out


def _slab(R, view="", **kw):
    """the frame on the forced slice-ring kernel without measured depth cuts, or None where it declines the pose"""
    R.set_option("kernel", 2)
    R.set_option("slab_split", 1)
    try:
        out = R.render(**kw)
    except Exception as e:      # SmkError: "... forced but not applicable: <a reason of the pose>"
        assert "not applicable" in str(e) and "u16" not in str(e), e
        return None
    finally:
        R.set_option("kernel", 0)
        R.set_option("slab_split", 0)
    assert R.last_frame_info()[0] == 2, "smk_last_frame_info does not show the forced kernel"
    assert R.stat("slab_status") == 0 and R.stat("slab_failures") == 0
    SLAB_RAN[view] = SLAB_RAN.get(view, 0) + 1
    return out


def _refused(R, smk, why, **opts):
    for k, v in opts.items():
        R.set_option(k, v)
    with pytest.raises(smk.SmkError) as e:
        R.render()
    assert why in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------------ parity with the checker

@pytest.mark.parametrize("c", U.PARITY, ids=U.parity_id)
def test_parity_with_the_checker(R, c):
    _, _, _, _, blend, depth, _ = c
    k = U.parity_case(c)
    ref = k.sc.render(blend=blend, depth=depth)
    U.push(R, k)
    R.set_blend(blend)
    got = _gather(R, depth=depth)
    slab = _slab(R, c[3], depth=depth)
    if depth:
        (ref, rdep), (got, dep) = ref, got
        hit = np.isfinite(rdep)
        assert hit.any() and np.array_equal(np.isfinite(dep), hit) and np.abs(dep[hit] - rdep[hit]).max() <= 1e-4
        if slab is not None:
            slab, sdep = slab
            assert np.array_equal(np.isfinite(sdep), hit) and np.array_equal(sdep[hit], dep[hit])
    assert ref[..., 3].max() > 0.05
    e = np.abs(got - ref).max()
    print("%s: max abs err against the checker %.3g" % (U.parity_id(c), e))
    assert e <= TOL, e
    if slab is not None:
        es, d = np.abs(slab - ref).max(), np.abs(slab - got).max()
        print("    slice ring: against the checker %.3g, against gather %.3g" % (es, d))
        assert es <= TOL, es
        if blend == 1:
            assert d <= TOL_REASSOC, d
        else:
            assert np.array_equal(slab, got), d


def test_fine_structure(R):
    """the scene test_u16_cpu.py qualifies: its 8-bit rendering is >= 1e-2 away, so only 16-bit voxels pass"""
    k = U.fine_case()
    ref = k.sc.render()
    U.push(R, k)
    got = _gather(R)
    e = np.abs(got - ref).max()
    e8 = np.abs(got - U.fine_case(eight_bit=True).sc.render()).max()
    print("fine structure: max abs err against the 16-bit frame %.3g, against the 8-bit frame %.3g" % (e, e8))
    assert e <= TOL, e
    assert e8 >= 1e-2
    slab = _slab(R, "rot")
    assert slab is not None and np.array_equal(slab, got)


# ------------------------------------------------------------------------------------------------ kernels

def test_kernel_choice_and_brick_flags(R, smk):
    k = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_EVEN)
    U.push(R, k)
    on, son = _gather(R), _slab(R, "rot")
    R.set_option("bricks", 0)
    off, soff = _gather(R), _slab(R, "rot")
    R.set_option("bricks", 1)
    assert np.array_equal(on, off), "the brick flags changed the frame"
    assert son is not None and soff is not None and np.array_equal(son, on) and np.array_equal(soff, on)
    assert np.abs(on - k.sc.render()).max() <= TOL
    # the column-stream kernel has no u16 instance: forced, it says so
    _refused(R, smk, NO_COLS, kernel=3)
    R.set_option("kernel", 0)
    # the automatic choice tries both ray-marchers (identical frames) and keeps one
    seen = set()
    for _ in range(12):
        assert np.array_equal(R.render(), on)
        seen.add(R.last_frame_info()[0])
        assert R.stat("slab_failures") == 0
    assert seen == {1, 2}, seen


def test_brick_flags_under_a_sparse_table(R):
    """cfg 3's widgets leave most of the table transparent: bricks are skipped, and no bit of the frame moves"""
    from _scenes import tf_cfg3
    k = U.case(2, "2d", shade=1, view="rot", dims=U.DIMS_33)
    k.sc.tf_vg = tf_cfg3()
    v = np.array(k.vol16)
    v[:, :, :17] = 0                                # (half the volume empty: bricks whose whole range is transparent)
    k = U.Case(v, L.with_data(k.sc, U.decode_u16(v)))
    U.push(R, k)
    on, son = _gather(R), _slab(R, "rot")
    flags, in_use = R.brick_flags()
    assert in_use and 0 < flags.sum() < flags.size, "vacuous: the flags skip nothing (or everything)"
    R.set_option("bricks", 0)
    off, soff = _gather(R), _slab(R, "rot")
    assert np.array_equal(on, off)
    assert son is not None and soff is not None and np.array_equal(son, on) and np.array_equal(soff, on)
    assert on[..., 3].max() > 0.05 and np.abs(on - k.sc.render()).max() <= TOL


# ------------------------------------------------------------------------------------------------ bricks and shards

def test_uneven_and_shuffled_bricks(gpu_renderer_factory):
    k = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_ODD)
    Rr = gpu_renderer_factory()
    try:
        U.push(Rr, k)
        whole, swhole = _gather(Rr), _slab(Rr, "rot")
        assert np.abs(whole - k.sc.render()).max() <= TOL
        assert swhole is not None and np.array_equal(swhole, whole)      # (odd rows are padded to even lengths)
        for grid in sorted(U.CUTS):
            n = grid[0] * grid[1] * grid[2]
            U.push(Rr, k, grid, L.shuffled(n))
            got = _gather(Rr)
            assert np.array_equal(got, whole), "bricks %s: %g" % (grid, np.abs(got - whole).max())
            assert np.array_equal(_slab(Rr, "rot"), whole)
    finally:
        Rr.close()


def test_upload_from_device_memory(gpu_renderer_factory):
    import torch
    k = U.case(2, "2d", shade=1, view="x+", dims=U.DIMS_ODD)

    def dev(a):
        t = torch.from_numpy(np.array(a).view(np.int16) if a.dtype == np.uint16 else np.array(a)).cuda()
        return t.data_ptr(), t
    Rr = gpu_renderer_factory()
    try:
        U.push(Rr, k, (3, 1, 2), L.shuffled(6))
        host = _gather(Rr)
        keep = U.upload(Rr, k, (3, 1, 2), L.shuffled(6), to_device=dev, ready=torch.cuda.synchronize)
        torch.cuda.synchronize()
        got = _gather(Rr)
        del keep
        assert np.array_equal(got, host) and np.abs(got - k.sc.render()).max() <= TOL
    finally:
        Rr.close()


def test_two_shards_with_halo(gpu_renderer_factory):
    """both ranks of a two-rank shard of the all-odd volume, bricked, merged as tests/test_gpu_sortlast.py merges them:
    within 2e-5 of the whole volume's frame, each rank's layer within the parity bound of the checker's"""
    import torch
    from simian_spacemonkey_amd import sortlast
    k = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_ODD)
    sc = k.sc
    world, npix = 2, sc.width * sc.height
    layers = torch.zeros((world, npix, 4), dtype=torch.float32, device="cuda")
    rs = []
    try:
        R0 = gpu_renderer_factory()
        rs.append(R0)
        U.push(R0, k)
        whole = _gather(R0)
        for r in range(world):
            Rr = gpu_renderer_factory()
            rs.append(Rr)
            Rr.set_shard(r, world)
            U.push(Rr, k, (3, 1, 2), L.shuffled(6))
            Rr.set_option("kernel", 1)
            Rr.render_device(layers[r].data_ptr(), None, None)
        torch.cuda.synchronize()
        order = rs[1].shard_order(world)
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        rs[1].composite_over_device(layers.data_ptr(), world, order, npix, out.data_ptr(), None)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(sc.height, sc.width, 4)
        assert whole[..., 3].max() > 0.05
        e = np.abs(got - whole).max()
        print("two shards against the whole: %.3g" % e)
        assert e <= 2e-5, e
        for r in range(world):
            part = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_ODD).sc
            part.region = sortlast.shard_region(sc.dims, r, world)
            pr = part.render()
            e = np.abs(layers[r].cpu().numpy().reshape(sc.height, sc.width, 4) - pr).max()
            assert pr[..., 3].max() > 0.05 and e <= TOL, (r, e)
    finally:
        for Rr in rs:
            Rr.close()


# ------------------------------------------------------------------------------------------------ time steps

def test_a_ring_of_three_u16_steps(gpu_renderer_factory, smk):
    ks = [U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_ODD, seed=s) for s in (3, 4, 5)]
    fresh = []
    for k in ks:                                    # what a fresh context renders of each step
        Rf = gpu_renderer_factory()
        try:
            U.push(Rf, k)
            fresh.append(_gather(Rf))
        finally:
            Rf.close()
    assert np.abs(fresh[0] - fresh[1]).max() > 1e-2 and np.abs(fresh[1] - fresh[2]).max() > 1e-2
    for f, k in zip(fresh, ks):
        assert np.abs(f - k.sc.render()).max() <= TOL
    Rr = gpu_renderer_factory()
    try:
        Rr.set_timestep_cache(3)
        U.push(Rr, ks[0])
        U.upload(Rr, ks[1], timestep=1)
        U.upload(Rr, ks[2], (2, 2, 2), L.shuffled(8), timestep=2)
        assert Rr.timesteps() == (0, [0, 1, 2])
        for t in (1, 2, 0, 2, 1, 0):
            Rr.select_timestep(t)
            assert np.array_equal(_gather(Rr), fresh[t]), t
            assert np.array_equal(_slab(Rr, "rot"), fresh[t]), t
        # a ring is of one type: a u8 step is refused, as a changed geometry is
        d8 = np.ascontiguousarray(U.q8(ks[0].vol16))
        descs, keep = U.descriptors(d8, ks[0].sc.grad, ks[0].sc.fsize)
        rc = Rr.L.smk_upload_timestep(Rr.ctx, 1, descs, len(descs), 3, 0, L.MODES.index("VGH"))
        msg = Rr.L.smk_last_error(Rr.ctx).decode()
        assert rc != 0 and "dtype 0 differs from the series' 2" in msg, msg
        Rr.select_timestep(1)
        assert np.array_equal(_gather(Rr), fresh[1])        # (the refused step changed nothing)
    finally:
        Rr.close()


# ------------------------------------------------------------------------------------------------ shadows (look 0)

@pytest.mark.parametrize("path", ["auto", "gather", "slice_ring"])
@pytest.mark.parametrize("table,shade", [("2d3", 1), ("3d", 0)])
def test_shadows(R, path, table, shade):
    k = U.case(3, table, shade=shade, view="rot", dims=U.DIMS_EVEN)
    sc = k.sc
    sc.light_pos = L.SHADOW_LIGHT
    sc.shadow = L.SHADOW
    ref, refL = sc.render_shadow()
    assert ref[..., 3].max() > 0.05 and refL[..., 3].max() > 0.05, "vacuous scene"
    U.push(R, k)
    R.set_option("kernel", {"auto": 0, "gather": 1, "slice_ring": 2}[path])
    got = R.render()
    gotL = R.light_buffer()
    assert R.last_frame_info()[0] in {"auto": (1, 2), "gather": (1,), "slice_ring": (2,)}[path]
    assert R.stat("slab_failures") == 0
    assert gotL.shape == refL.shape
    eL, e = np.abs(gotL - refL).max(), np.abs(got - ref).max()
    print("shadows %s %s: frame %.3g, light buffer %.3g" % (table, path, e, eL))
    assert eL <= TOL, "light buffer max abs err %g" % eL
    assert e <= TOL, "frame max abs err %g" % e


def test_shadow_paths_left_out_are_refused(R, smk):
    k = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_EVEN)
    k.sc.light_pos, k.sc.shadow = L.SHADOW_LIGHT, L.SHADOW
    U.push(R, k)
    why = "u16 voxels render shadows with the two marches only"
    _refused(R, smk, why, shadow_march=0)
    R.set_option("shadow_march", 1)
    _refused(R, smk, why, shadow_fused=1)
    R.set_option("shadow_fused", 0)
    _refused(R, smk, "column-stream kernel has no shadow mode", kernel=3)


def test_slice_ring_instances_left_out_are_refused(R, smk):
    """scene depth and the NV20 look: a forced slice-ring kernel says why, the automatic choice renders on the gather kernel"""
    k = U.case(3, "2d3", shade=2, view="rot", dims=U.DIMS_EVEN)
    sc = k.sc
    U.push(R, k)
    zs = np.full((sc.height, sc.width), 7.0, np.float32)
    want = _gather(R, scene_depth=zs)
    assert np.abs(want - _gather(R)).max() > 1e-2, "vacuous: the scene depth hides nothing"
    R.set_option("kernel", 2)
    with pytest.raises(smk.SmkError) as e:
        R.render(scene_depth=zs)
    assert NO_OCC in str(e.value), str(e.value)
    R.set_option("kernel", 0)
    for _ in range(3):
        assert np.array_equal(R.render(scene_depth=zs), want) and R.last_frame_info()[0] == 1
    sc.light_pos, sc.shadow = L.SHADOW_LIGHT, L.SHADOW
    U.frame_state(R, sc)
    R.set_option("shadow_look", 1)
    _refused(R, smk, NO_NV20, kernel=2)
    R.set_option("kernel", 0)
    look1 = R.render()
    assert R.last_frame_info()[0] == 1 and look1[..., 3].max() > 0.05
    # the NV20 look through the eye pass that exists (the gather kernel's): the frame of the decoded voxels uploaded as f32
    R.upload_volume(sc.data, sc.grad, fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
    R.set_option("kernel", 1)
    as_f32 = R.render()
    assert np.abs(look1 - as_f32).max() <= TOL
    R.set_shadow(0)
    assert np.abs(R.render() - look1).max() > 1e-3, "vacuous: the shadows darken nothing"


# ------------------------------------------------------------------------------------------------ perturbation, the slices

def test_perturbed_fetch(R):
    import oracle as O
    k = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_EVEN)
    sc = k.sc
    sc.noise, sc.pert_w, sc.pert_s = O.noise_tex(32), (.2, .1, 0, 0), (.2, 2.1, 4.5, 8.7)
    ref = sc.render()
    plain = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_EVEN).sc.render()
    assert np.abs(ref - plain).max() > 1e-2, "vacuous: the noise moves nothing"
    U.push(R, k)
    R.set_perturb(sc.noise, sc.pert_w, sc.pert_s)
    got = R.render()
    assert R.last_frame_info()[0] == 1
    e = np.abs(got - ref).max()
    print("perturbed: %.3g" % e)
    assert e <= TOL, e


@pytest.mark.parametrize("nelts", [1, 3])
def test_slice_quad(R, nelts):
    """smk_render_slice called directly, against the float64 quad of oracle/gl_slices.py over the decoded volume"""
    k = U.case(nelts, "2d", shade=0, view="rot", window=(37, 29), dims=U.DIMS_ODD)
    sc = k.sc
    base = sc.render()
    U.push(R, k)
    quads = L.quads(sc)
    for name in ("oblique", "axis", "outside", "behind"):
        for alpha in (0.6, 2.5):
            want, edge = L.slice_reference(sc, base, quads[name], alpha)
            got = R.render_slice(quads[name], alpha, base.copy())
            inner = ~edge
            assert edge.sum() < 0.1 * inner.sum()
            if name in L.NO_DRAW:
                assert np.array_equal(got, base)
            else:
                assert np.abs(want - base).max() > 0.05
                e = np.abs(got[inner] - want[inner]).max()
                assert e <= TOL, (name, alpha, e)


@pytest.mark.parametrize("oaxis,look", [(5, "r8k"), (1, "nv20"), (1, "r8k")])
def test_clip_widget_slice(R, oaxis, look):
    """the clip-plane widget's data slice against tests/_clip_slice_ref.py on the decoded volume (frames, poses and bounds
    of tests/test_gpu_clip_slice.py)"""
    import _clip_slice_ref as CS
    from _clip_slice_cases import CASE_POSE, PASS_TABLE, SIZE, clip_vpos, widget_corners
    from _scenes import POSES
    import oracle as O
    k = U.case(3, "2d3", shade=1, view="rot", window=(SIZE, SIZE), dims=(32, 32, 32))
    sc = k.sc
    name = CASE_POSE[oaxis]
    sc.xform = {"rot": O.rotation((1, 1, 0), 30), "side": O.rotation((.2, 1, .1), 75)}.get(name) or O.rotation(*POSES[name])
    vpos = clip_vpos(oaxis, sc.fsize, 0.45)
    corners = widget_corners(oaxis, vpos, sc.fsize, 0.25)
    U.push(R, k)
    R.set_clip(oaxis, vpos)
    V = _gather(R)
    assert V[..., 3].max() > 0.05
    S, cover, _ = CS.slice_layer(sc.data, "VGH", sc.fsize, sc.mv(), sc.frustum, sc.znear, sc.width, sc.height, corners, oaxis,
                                 0.6, look)
    edge = CS.edge_pixels(CS.moved_quad(corners, sc.fsize, oaxis), sc.mv(), sc.frustum, sc.znear, 20.0, sc.width, sc.height)
    assert cover.sum() > 300 and edge.sum() <= 1e-3 * cover.sum()
    keep = ~edge
    for dv, want_pass in ((-0.5, PASS_TABLE[oaxis][0]), (0.5, PASS_TABLE[oaxis][1])):
        R.set_clip_slice(corners, 0.6, dv, look)
        got = _gather(R)
        assert R.stat("clip_slice_pass") == want_pass
        want = CS.compose(V, S, cover, want_pass)
        e = np.abs(got.astype(np.float64) - want)[keep].max()
        assert e <= TOL, (dv, e)
        assert np.array_equal(got[~cover & keep], V[~cover & keep])
        assert np.abs(got - V)[cover & keep].max() > 1e-3, "vacuous: the slice changes nothing"


def test_count_samples(R):
    """smk_count_samples against the checker's count of the same frame (it marches every plane of every ray)"""
    import oracle as O
    k = U.case(2, "2d", dims=U.DIMS_ODD)
    k.sc.render()
    want = O.inside_samples()
    U.push(R, k)
    assert want > 0 and R.count_samples() == want


def test_slice_ring_instances_that_would_spill_are_left_out(R, smk):
    """NV20 shading under the dense 3-D table with brick flags on the 10+2-wave shapes (option tile 20: 40 x 16 pixels): not
    built (smk_slab.h slab_inst_missing); forced, the kernel says so; its own choice passes the shape over"""
    from _scenes import tf3d_panes
    k = U.case(3, "3d", shade=2, view="rot", dims=U.DIMS_EVEN)
    k.sc.tf3d = tf3d_panes()
    v = np.array(k.vol16)
    v[:, :, :16] = 0                                # (half the volume empty: the brick flags stay in use)
    k = U.Case(v, L.with_data(k.sc, U.decode_u16(v)))
    U.push(R, k)
    want = _gather(R)
    assert R.brick_flags()[1], "vacuous: the frame has no brick flags"
    assert want[..., 3].max() > 0.05 and np.abs(want - k.sc.render()).max() <= TOL
    try:
        R.set_option("tile", 20)
        _refused(R, smk, "u16 voxels have no 10+2-wave instances with NV20 shading, the 3-D table and brick flags", kernel=2)
        R.set_option("bricks", 0)                   # (without brick flags the shape has its instance)
        got = _slab(R, "rot")
        assert got is not None and (R.stat("slab_plan_tw"), R.stat("slab_plan_th")) == (40, 16) and np.array_equal(got, want)
        R.set_option("bricks", 1)
        R.set_option("tile", 0)
        got = _slab(R, "rot")
        assert got is not None and np.array_equal(got, want)
        assert (R.stat("slab_plan_tw"), R.stat("slab_plan_th")) not in ((40, 16), (16, 40))
    finally:
        R.set_option("tile", 0)


def test_the_slice_ring_kernel_took_part():
    """(runs after the cases above) a forced slice-ring kernel may decline a pose; it must have rendered views of both
    principal-axis families, the x-major copy's among them"""
    assert sum(SLAB_RAN.values()) >= 16, SLAB_RAN
    assert any(v.startswith("x") for v in SLAB_RAN) and any(not v.startswith("x") for v in SLAB_RAN), SLAB_RAN


# ------------------------------------------------------------------------------------------------ refusals

def test_four_channels_are_refused(R):
    d = np.zeros((4, 4, 4, 4), np.uint16)
    descs, keep = U.descriptors(d, None, (1.0, 1.0, 1.0))
    rc = R.L.smk_upload_volume(R.ctx, descs, 1, 4, 2, L.MODES.index("V4"))
    msg = R.L.smk_last_error(R.ctx).decode()
    assert rc != 0 and "4-channel u16 voxels" in msg, msg
    rc = R.L.smk_upload_timestep(R.ctx, 0, descs, 1, 4, 2, L.MODES.index("V4"))
    assert rc != 0 and "4-channel u16 voxels" in R.L.smk_last_error(R.ctx).decode()


# ------------------------------------------------------------------------------------------------ quantise and prep

def test_quantize_u16_device(R):
    import torch
    rng = np.random.default_rng(7)
    f = np.float32
    edge = np.array([np.nan, np.inf, -np.inf, -1.0, -1e-30, -0.0, 0.0, 1.0, 1.5, 0.5, 1.5 / 65535, 2.5 / 65535, 0.49 / 65535,
                     np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)), 65534.4 / 65535, 3e38, 1e-45], np.float32)
    halves = ((np.arange(1, 4001) + .5) / 65535.0).astype(np.float32)
    v = np.concatenate([edge, halves, rng.random(40000 - edge.size - halves.size - 2000, dtype=np.float32),
                        (rng.normal(size=2000) * 2).astype(np.float32)])
    assert v.size == 40000
    want = U.quantize_u16(v)
    assert want.min() == 0 and want.max() == 65535 and len(np.unique(want)) > 10000
    src = torch.from_numpy(v).cuda()
    dst = torch.full((v.size + 8,), -1, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    R.quantize_u16_device(src.data_ptr(), v.size, dst.data_ptr())
    out = dst.cpu().numpy()
    assert (out[v.size:] == -1).all(), "wrote past n_values"
    got = out[:v.size].view(np.uint16)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5], v[bad[:5]], got[bad[:5]], want[bad[:5]])
    rc = R.L.smk_quantize_u16_device(R.ctx, None, 4, ctypes.c_void_p(dst.data_ptr()))
    assert rc != 0 and "smk_quantize_u16_device: bad arguments" in R.L.smk_last_error(R.ctx).decode()


@pytest.mark.parametrize("compat", [0, 1])
def test_make_vgh_from_u16_is_the_f32_call(R, compat):
    import torch
    dims = (23, 17, 13)
    d, _ = U.volume16(U.DIMS_ODD)
    s16 = np.ascontiguousarray(d[:dims[2], :dims[1], :dims[0], 0])
    n = s16.size
    a16 = torch.from_numpy(s16.view(np.int16)).cuda()
    a32 = torch.from_numpy(s16.astype(np.float32)).cuda()
    outs = []
    for src, dt in ((a16, 2), (a32, 1)):
        o8 = torch.zeros(n * 3, dtype=torch.uint8, device="cuda")
        of = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        R.make_vgh_device(src.data_ptr(), dt, dims, compat, o8.data_ptr(), of.data_ptr())
        outs.append((o8.cpu().numpy(), of.cpu().numpy()))
    assert outs[1][0].max() > 200 and outs[1][1].max() > 0.9, "vacuous"
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))


def test_float_prep_to_u16_voxels(R):
    """the bridge the entry is for: smk_make_vgh_device's f32 output, quantised on the device, uploaded from device memory
    as SMK_U16 -- the frame is the checker's of the decoded voxels"""
    import torch
    import oracle as O
    dims = U.DIMS_EVEN
    d, nrm = U.volume16(dims)
    n = d.shape[0] * d.shape[1] * d.shape[2]
    a16 = torch.from_numpy(np.ascontiguousarray(d[..., 0]).view(np.int16)).cuda()
    of = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
    q = torch.zeros(n * 3, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    R.make_vgh_device(a16.data_ptr(), 2, dims, 0, None, of.data_ptr())
    R.quantize_u16_device(of.data_ptr(), n * 3, q.data_ptr())
    vol16 = q.cpu().numpy().view(np.uint16).reshape(d.shape)
    assert np.array_equal(vol16, U.quantize_u16(of.cpu().numpy()).reshape(d.shape))
    sc = O.Scene(U.decode_u16(vol16), grad=nrm)
    sc.tf_mode, sc.tf_vg, sc.tf_h, sc.tf3d = L.tables("2d3")
    sc.dmode, sc.third_axis = "VGH", 1
    sc.width = sc.height = 48
    sc.steps = 48
    sc.shade_mode = 1
    L.pose(sc, "rot")
    g = torch.from_numpy(np.array(nrm)).cuda()
    torch.cuda.synchronize()
    R.upload_volume_device(q.data_ptr(), dims, 3, 2, grad_dptr=g.data_ptr(), fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
    U.frame_state(R, sc)
    got = _gather(R)
    ref = sc.render()
    assert ref[..., 3].max() > 0.05 and np.abs(got - ref).max() <= TOL


# ------------------------------------------------------------------------------------------------ the Python binding

def test_binding_takes_uint16_and_refuses_other_types(R):
    k = U.case(3, "2d3", shade=1, view="rot", dims=U.DIMS_EVEN)
    sc = k.sc
    U.push(R, k)
    want = _gather(R)
    R.upload_volume(k.vol16, sc.grad, fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
    got = _gather(R)
    assert np.array_equal(got, want) and np.abs(got - sc.render()).max() <= TOL
    for bad in (np.int16, np.float64, np.int32):
        with pytest.raises(TypeError):
            R.upload_volume(k.vol16.astype(bad), sc.grad, dmode="VGH")
    with pytest.raises(TypeError):
        R.upload_timestep(1, k.vol16.astype(np.int16), sc.grad, dmode="VGH")
    assert np.array_equal(_gather(R), want)         # (a refused array changed nothing)
