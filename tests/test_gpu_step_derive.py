"""Derivatives of a step (smk.h smk_derive_timestep, smk_upload_timestep_scalar_device): the step made inside the ring must
be, bit for bit, the step a FRESH context holds after it uploaded what the recipe "Derivatives of a blend" makes of the same
scalar with the existing device entries (smk_make_vgh_device, smk_quantize_u16_device, smk_normals_*_device) in the same
test -- voxels and normals as smk_download_timestep returns them, frames on the gather and the slice-ring kernel, the step
histogram.  Where the scalar is finite the arrays are also the CPU checker's (tests/_step_derive_ref.py, qualified by
tests/test_step_derive_cpu.py; more of that in tests/test_gpu_step_derive_shapes.py).  Volumes are 37 x 13 x 11 and
70 x 21 x 19 voxels and smaller."""
import os
import subprocess

import numpy as np
import pytest

import _step_derive_ref as V
import _tblend_ref as T
from _gpu_mem import dev_ptr as dev, out_buffer, stream_arg
from _step_gpu import RAN, Undisturbed, recipe, recipe_download, same_bits as same, scene_context, series
from _trex_series import write_series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = dict(ids=lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else None)


# ---- 1. equals the recipe

@pytest.mark.parametrize("compat, blur", V.CASES)
@pytest.mark.parametrize("dims", V.DIMS, **IDS)
@pytest.mark.parametrize("ring", V.RINGS)
def test_derive_of_a_blend_equals_the_recipe(gpu_renderer_factory, O, ring, dims, compat, blur):
    a, b, mixed = V.blended(O, dims, ring)
    R = series(gpu_renderer_factory, (a, b))
    try:
        R.blend_timesteps(0, 1, V.W, 2)
        R.derive_timestep(2, 3, compat, blur)
        assert R.timesteps() == (0, [0, 1, 2, 3])           # (a derived step does not become current)
        got = R.download_timestep(3)
        bl = R.download_timestep(2)
        same(bl[0], V.downloaded(*mixed)[0], "the blend")
        s = np.ascontiguousarray(bl[0][..., 0])             # the blended SCALAR, as the recipe reads it back
        want = recipe_download(gpu_renderer_factory, R, s, ring, compat, blur)
        same(R.download_timestep(2)[0], bl[0], "the source, afterwards")
    finally:
        R.close()
    same(got[0], want[0], "data")
    same(got[1], want[1], "normals")
    assert not np.array_equal(got[0][..., 0], s) and got[0][..., 1:].any() and (got[1] != 128).any()
    if np.isfinite(s.astype(np.float64)).all():             # ... and the CPU checker's arrays
        ref = V.downloaded(*V.derive(O, s, ring, compat, blur))
        same(got[0], ref[0], "data against the checker")
        same(got[1], ref[1], "normals against the checker")


# ---- 2. frames and summaries

def high_g_table():
    """a 2-D table [g][v] that shows only voxels of high gradient magnitude: a wrong brick summary drops their samples"""
    tex = np.zeros((256, 256, 4), np.uint8)
    tex[150:, :, 0] = np.arange(256, dtype=np.uint8)[None, :]
    tex[150:, :, 1] = 255 - np.arange(256, dtype=np.uint8)[None, :]
    tex[150:, :, 2] = 90
    tex[150:, :, 3] = 200
    return tex


def high_g_scene(data, grad):
    sc = T.scene(data, grad)
    sc.tf_vg = high_g_table()
    return sc


@pytest.mark.parametrize("kernel", [1, 2], ids=["gather", "slice-ring"])
@pytest.mark.parametrize("ring", V.RINGS)
def test_a_derived_step_renders_and_counts_like_the_recipes_upload(gpu_renderer_factory, O, ring, kernel):
    from _scenes import push_scene
    dims = V.DIMS[0]
    a, b, _ = V.blended(O, dims, ring)
    opts = (("kernel", kernel), ("bricks", 1))
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(4)
        push_scene(R, high_g_scene(*a))
        for k, v in opts:
            R.set_option(k, v)
        R.upload_timestep(1, b[0], b[1], fsize=tuple(float(f) for f in high_g_scene(*a).fsize), dmode="VGH")
        R.render()
        R.blend_timesteps(0, 1, V.W, 2)
        R.derive_timestep(2, 3, 1, 0)
        R.select_timestep(3)
        got = R.render()
        assert R.last_frame_info()[0] == RAN[kernel]
        assert R.brick_flags()[1], "brick flags are not in use"
        flags = R.brick_flags()[0]
        counts = R.hist2d_step(3)
        s = np.ascontiguousarray(R.download_timestep(2)[0][..., 0])
        data, nrm = recipe(R, s, ring, 1, 0)
        assert R.stat("slab_failures") == 0
    finally:
        R.close()
    F = gpu_renderer_factory()
    try:
        push_scene(F, high_g_scene(data, nrm))
        for k, v in opts:
            F.set_option(k, v)
        want = F.render()
        assert F.last_frame_info()[0] == RAN[kernel]
        wflags = F.brick_flags()[0]
        wcounts = F.hist2d_step()
    finally:
        F.close()
    assert want[..., 3].max() > 0.05 and 0 < int((wflags != 0).sum())
    assert np.array_equal(flags, wflags), "brick flags"
    assert np.array_equal(counts, wcounts), "step histogram"
    assert np.array_equal(got, want), "frame: max diff %g" % np.abs(got - want).max()


# ---- 3. edge shapes

def edge_scalars():
    rng = np.random.default_rng(5)
    one = rng.integers(0, 256, (3, 3, 3), dtype=np.uint8)
    thin = rng.integers(0, 256, (3, 4, 5), dtype=np.uint8)                # 5 x 4 x 3
    const = np.full((6, 5, 7), 93, np.uint8)
    return {"3x3x3": one, "5x4x3": thin, "constant": const}


# (integer voxels hold no NaN: a float scalar with one goes into those rings in test_scalar_form)
EDGES = [(n, r) for n in ("3x3x3", "5x4x3", "constant", "5x4x3-no-normals") for r in V.RINGS] + [("nonfinite", "f32")]


@pytest.mark.parametrize("name, ring", EDGES)
def test_edge_shapes_equal_the_recipe(gpu_renderer_factory, name, ring):
    normals = not name.endswith("no-normals")
    if name == "nonfinite":                                 # a NaN and an infinity in the scalar: a float ring keeps them
        s = V.as_type(V.scalar(0, (9, 7, 6)), "f32").copy()
        s[2, 3, 4], s[3, 2, 6] = np.nan, np.inf
    else:
        s = V.as_type(edge_scalars()[name.replace("-no-normals", "")], ring)
    nz, ny, nx = s.shape
    data = np.zeros((nz, ny, nx, 3), s.dtype)
    data[..., 0] = s
    data[..., 1] = s[::-1]                                  # (what the source holds beside channel 0 is not read)
    grad = np.full((nz, ny, nx, 3), 7, np.uint8) if normals else None
    for compat, blur in V.CASES:
        R = series(gpu_renderer_factory, ((data, grad),), cap=2)
        try:
            R.derive_timestep(0, 1, compat, blur)
            got = R.download_timestep(1)
            want = recipe_download(gpu_renderer_factory, R, s, ring, compat, blur, normals=normals)
        finally:
            R.close()
        same(got[0], want[0], "%s %s: data" % (name, ring))
        same(got[1], want[1], "%s %s: normals" % (name, ring))
        if not normals:
            assert (got[1] == 128).all()


# ---- 4. the scalar form

@pytest.mark.parametrize("ring", V.RINGS)
@pytest.mark.parametrize("kind", V.RINGS)
def test_scalar_form(gpu_renderer_factory, O, kind, ring):
    """a dense scalar of type `kind` from device memory into a ring of type `ring`"""
    dims = V.SMALL
    a = V.series_step(O, V.scalar(0, dims), ring)
    s = V.as_type(V.scalar(1, dims), kind)
    if kind == "f32":
        s = s.copy()
        s[5, 6, 20], s[4, 4, 30] = np.nan, -np.inf
    esz = s.dtype.itemsize
    shifts = {"u8": (0, 1), "u16": (0, 2), "f32": (0, 4)}[kind]             # an odd address; one that is 2 mod 4
    for (compat, blur), shift in zip(V.CASES, shifts):
        R = series(gpu_renderer_factory, (a,), cap=2)
        try:
            ps, keep = dev(s, shift)
            assert ps % 256 == shift and ps % esz == 0
            R.upload_timestep_scalar_device(4, ps, V.CODE[kind], dims, compat, blur)
            assert R.timesteps() == (0, [0, 4])
            got = R.download_timestep(4)
            want = recipe_download(gpu_renderer_factory, R, s, ring, compat, blur)
            same(R.download_timestep(0)[0], V.downloaded(*a)[0], "the current step")
        finally:
            R.close()
        same(got[0], want[0], "%s into %s: data" % (kind, ring))
        same(got[1], want[1], "%s into %s: normals" % (kind, ring))
        if np.isfinite(s.astype(np.float64)).all():         # (the checker has no contract for a NaN in the scalar)
            ref = V.downloaded(*V.derive(O, s, ring, compat, blur))
            same(got[0], ref[0], "data against the checker")
            same(got[1], ref[1], "normals against the checker")


# ---- 5. ordering

def test_derive_on_a_second_stream_behind_a_blend_and_a_source_overwritten(gpu_renderer_factory, O):
    import torch
    from _scenes import push_scene
    dims, ring = V.SMALL, "u8"
    a, b, _ = V.blended(O, dims, ring)
    c = V.series_step(O, V.scalar(2, dims), ring)
    sca = T.scene(*a)
    R = gpu_renderer_factory()
    try:                                                    # the synchronous results
        R.set_timestep_cache(4)
        push_scene(R, sca)
        R.upload_timestep(1, b[0], b[1], fsize=tuple(float(f) for f in sca.fsize), dmode="VGH")
        want0 = R.render()
        R.blend_timesteps(0, 1, V.W, 2)
        R.derive_timestep(2, 3, 1, 1)
        want = R.download_timestep(3)
        R.select_timestep(3)
        want3 = R.render()
        assert not np.array_equal(want0, want3) and want3[..., 3].max() > 0.05
    finally:
        R.close()
    rend, bl, dv, up = (torch.cuda.Stream() for _ in range(4))
    pc, kc = dev(c[0])
    pg, kg = dev(c[1])
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(4)
        push_scene(R, sca)
        R.upload_timestep(1, b[0], b[1], fsize=tuple(float(f) for f in sca.fsize), dmode="VGH")
        torch.cuda.synchronize()                            # nothing is in flight when the four streams start
        outs = []

        def frames(n, t):
            for _ in range(n):
                o = torch.empty((sca.height, sca.width, 4), dtype=torch.float32, device="cuda")
                outs.append((o, t))
                R.render_device(o.data_ptr(), None, stream_arg(rend))
        frames(12, 0)                                       # frames of step 0 in flight ...
        R.blend_timesteps(0, 1, V.W, 2, stream=stream_arg(bl))
        R.derive_timestep(2, 3, 1, 1, stream=stream_arg(dv))               # ... directly behind the blend, no host wait
        R.upload_timestep_device(2, pc, dims, 3, 0, pg, fsize=tuple(float(f) for f in sca.fsize), dmode="VGH",
                                 stream=stream_arg(up))     # the source slot overwritten: behind the derive's reads
        R.select_timestep(3)
        frames(3, 3)
        R.derive_timestep(2, 3, 1, 0, stream=stream_arg(dv))               # into the slot those three read: it waits for them
        R.derive_timestep(1, 3, 1, 1, stream=stream_arg(bl))               # ... and again, on another stream
        torch.cuda.synchronize()                            # all four streams: read-back
        for i, (o, t) in enumerate(outs):
            assert np.array_equal(o.cpu().numpy(), want3 if t == 3 else want0), "frame %d (step %d)" % (i, t)
        same(R.download_timestep(2)[0], c[0], "the new step 2")
        R.blend_timesteps(0, 1, V.W, 2)
        R.derive_timestep(2, 3, 1, 1)
        got = R.download_timestep(3)
        assert R.stat("slab_failures") == 0
    finally:
        R.close()
    same(got[0], want[0], "data")
    same(got[1], want[1], "normals")


def test_async_results_equal_the_synchronous_ones(gpu_renderer_factory, O):
    """the download itself enqueued behind the derive on a third stream: nothing waits on the host before the end"""
    import torch
    dims, ring = V.SMALL, "f32"
    a, b, _ = V.blended(O, dims, ring)
    c = V.series_step(O, V.scalar(2, dims), ring)
    R = series(gpu_renderer_factory, (a, b))
    try:
        R.blend_timesteps(0, 1, V.W, 2)
        R.derive_timestep(2, 3, 0, 1)
        want = R.download_timestep(3)
    finally:
        R.close()
    nx, ny, nz = dims
    bl, dv, up, dn = (torch.cuda.Stream() for _ in range(4))
    pc, kc = dev(c[0])
    pg, kg = dev(c[1])
    out_d = out_buffer(nx * ny * nz * 3, np.float32)
    out_g = out_buffer(nx * ny * nz * 3, np.uint8)
    work = out_buffer(1 << 22, np.float32)
    R = series(gpu_renderer_factory, (a, b))
    try:
        torch.cuda.synchronize()                            # nothing is in flight when the four streams start
        with torch.cuda.stream(bl):                         # work in front of the blend: nothing behind it has started yet
            for _ in range(24):
                work.add_(1)
        R.blend_timesteps(0, 1, V.W, 2, stream=stream_arg(bl))
        R.derive_timestep(2, 3, 0, 1, stream=stream_arg(dv))
        R.upload_timestep_device(2, pc, dims, 3, 1, pg, dmode="VGH", stream=stream_arg(up))
        R.download_timestep_device(out_d.data_ptr(), out_g.data_ptr(), 3, stream_arg(dn))
        torch.cuda.synchronize()                            # all four streams: read-back
        same(out_d.cpu().numpy().reshape(nz, ny, nx, 3), want[0], "data")
        same(out_g.cpu().numpy().reshape(nz, ny, nx, 3), want[1], "normals")
        same(R.download_timestep(2)[0], c[0], "the new step 2")
    finally:
        R.close()


# ---- 6. ring and refusals

def test_ring_and_refusals(gpu_renderer_factory, smk, O):
    dims, ring = V.SMALL, "u8"
    nx, ny, nz = dims
    a, b, _ = V.blended(O, dims, ring)
    buf = out_buffer(nx * ny * nz * 4 + 64, np.uint8)
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match="smk_derive_timestep: no volume"):
            R.derive_timestep(0, 1)
        with pytest.raises(smk.SmkError, match="smk_upload_timestep_scalar_device: no volume"):
            R.upload_timestep_scalar_device(1, buf.data_ptr(), 0, dims)
    finally:
        R.close()
    sa = V.downloaded(*V.derive(O, np.ascontiguousarray(a[0][..., 0]), ring))
    sb = V.downloaded(*V.derive(O, np.ascontiguousarray(b[0][..., 0]), ring))
    # capacity 2: the source and the output, when the source is current
    sca = T.scene(*a)
    fsize = tuple(float(f) for f in sca.fsize)
    R = scene_context(gpu_renderer_factory, sca, cap=2)
    try:
        R.upload_timestep(1, b[0], b[1], fsize=fsize, dmode="VGH")
        with Undisturbed(R):                                # a refused call changes nothing: frames, flags, steps
            for args, why in (((99, 5), r"99 \(the source\) is not cached"), ((-1, 5), "is not cached"), ((0, -1), ">= 0"),
                              ((1, 1), "in-place"), ((1, 5), "holds 2 steps.*here 3")):
                with pytest.raises(smk.SmkError, match=why):
                    R.derive_timestep(*args)
            for args, why in (((5, None, 0, dims), "d_scalar is NULL"), ((5, buf.data_ptr(), 7, dims), "scalar_dtype 7"),
                              ((5, buf.data_ptr(), 0, (nx, ny + 1, nz)), "differ from the series'"),
                              ((5, buf.data_ptr() + 1, 2, dims), "not aligned to its 2-byte"),
                              ((5, buf.data_ptr() + 2, 1, dims), "not aligned to its 4-byte"), ((-3, buf.data_ptr(), 0, dims), ">= 0")):
                with pytest.raises(smk.SmkError, match=why):
                    R.upload_timestep_scalar_device(*args)
        assert R.timesteps() == (0, [0, 1])
        same(R.download_timestep(1)[0], b[0], "step 1 after the refusals")
        R.derive_timestep(0, 5)                             # the only slot that is neither the source's nor current: step 1's
        assert R.timesteps() == (0, [0, 5])
        same(R.download_timestep(5)[0], sa[0], "capacity 2")
        R.upload_timestep_scalar_device(6, dev(np.ascontiguousarray(b[0][..., 0]))[0], 0, dims)
        assert R.timesteps() == (0, [0, 6])
        same(R.download_timestep(6)[1], sb[1], "capacity 2, scalar form")
    finally:
        R.close()
    # capacity 3: a current step that is not the source is a third slot
    R = series(gpu_renderer_factory, (a, b), cap=3)
    try:
        R.derive_timestep(1, 5)
        assert R.timesteps() == (0, [0, 1, 5])
        R.derive_timestep(1, 6)                             # no empty slot: the one behind the last written, past the
        assert R.timesteps() == (0, [0, 1, 6])              # current step's and the source's
        same(R.download_timestep(6)[0], sb[0], "capacity 3")
        R.derive_timestep(0, 6, 0, 1)                       # a cached output is overwritten in place
        assert R.timesteps() == (0, [0, 1, 6])
        R.select_timestep(6)
        R.derive_timestep(1, 6)                             # ... the current step too
        assert R.timesteps() == (6, [0, 1, 6])
        same(R.download_timestep()[0], sb[0], "the current step overwritten")
        same(R.download_timestep()[1], sb[1], "the current step overwritten: normals")
    finally:
        R.close()
    # capacity 4: blend and derive beside the two ends
    R = series(gpu_renderer_factory, (a, b), cap=4)
    try:
        R.blend_timesteps(0, 1, V.W, 2)
        R.derive_timestep(2, 3)
        assert R.timesteps() == (0, [0, 1, 2, 3])
        R.derive_timestep(2, 7)                             # behind slot 3 comes slot 0, current: slot 1 goes
        assert R.timesteps() == (0, [0, 2, 3, 7])
        same(R.download_timestep(7)[0], R.download_timestep(3)[0], "capacity 4")
    finally:
        R.close()
    # a series that is not V, G, H; a sharded context
    two = np.ascontiguousarray(a[0][..., :2])
    R = scene_context(gpu_renderer_factory, T.scene(two, a[1]), cap=3)
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match="nelts 2"):
                R.derive_timestep(0, 1)
            with pytest.raises(smk.SmkError, match="nelts 2"):
                R.upload_timestep_scalar_device(1, buf.data_ptr(), 0, dims)
        same(R.download_timestep()[0], two, "after the refusals")
    finally:
        R.close()
    R = scene_context(gpu_renderer_factory, sca, cap=3, shard=(0, 2))
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match="sharded context.*2 voxels beyond.*whole volume's extremes"):
                R.derive_timestep(0, 1)
            with pytest.raises(smk.SmkError, match="sharded context"):
                R.upload_timestep_scalar_device(1, buf.data_ptr(), 0, dims)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    # a cache of one step -- a context that never asked for a series -- holds the current step and no other: no slot
    R = scene_context(gpu_renderer_factory, sca)
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match="smk_upload_timestep_scalar_device: time step 5: the cache holds one step, the current one"):
                R.upload_timestep_scalar_device(5, buf.data_ptr(), 0, dims)
            with pytest.raises(smk.SmkError, match="smk_derive_timestep: the cache holds 1 steps.*here 2"):
                R.derive_timestep(0, 5)
    finally:
        R.close()
    # a volume thinner than 3 voxels has no interior voxel (smk_make_vgh_device refuses it too)
    thin = (np.ascontiguousarray(a[0][:2]), np.ascontiguousarray(a[1][:2]))
    R = scene_context(gpu_renderer_factory, T.scene(*thin), cap=3)
    try:
        with Undisturbed(R, visible=False):                 # (two slices of voxels: whatever the frame shows, it stays)
            with pytest.raises(smk.SmkError, match="smk_derive_timestep: a 37x13x2 volume has no interior voxel"):
                R.derive_timestep(0, 1)
            with pytest.raises(smk.SmkError, match="smk_upload_timestep_scalar_device: a 37x13x2 volume has no interior voxel"):
                R.upload_timestep_scalar_device(1, buf.data_ptr(), 0, (nx, ny, 2))
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    assert not buf.any()


# ---- 7. the host adapter

def test_host_adapter_shows_the_derivatives_of_a_blend(tmp_path, O):
    """tests/host/derive_main drives HipVolumeRenderable::setTimeFraction + setTimeFractionDerivatives over a 3-step u8
    series: with derivatives on the step a fractional frame shows is the checker's VGH and normals of the blended scalar;
    with them off its frames are tblend_main's"""
    exe = os.path.join(ROOT, "tests", "host", "derive_main")
    tblend = os.path.join(ROOT, "tests", "host", "tblend_main")
    for e in (exe, tblend):
        assert os.path.exists(e), "%s is not built: __graft_entry__.build() builds it" % e
    dims = V.SMALL
    nx, ny, nz = dims
    steps = [V.series_step(O, V.scalar(s, dims), "u8") for s in (0, 1, 2)]
    d = tmp_path / "vgh"
    d.mkdir()
    for t, (data, nrm) in enumerate(steps):
        data.tofile(str(d / ("s.%d.vgh" % t)))
        nrm.tofile(str(d / ("s.%d.nrm" % t)))
    high_g_table().tofile(str(d / "table.rgba"))
    spec = "vgh:%s:%d:%d:%d:3:%s" % (d / "s", nx, ny, nz, d / "table.rgba")
    seq = "0:0,0:0.37,0:0.37,1:0.37,1:0"

    def run(prog, args, name, where):
        p = subprocess.run([prog] + args + [str(where / name)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        n = sum(line.startswith("frame ") for line in p.stdout.splitlines())
        return [np.fromfile("%s.%d.f32" % (where / name, k), np.float32) for k in range(n)], p.stderr

    def shown(name, k):
        return (np.fromfile("%s.%d.data" % (d / name, k), np.uint8).reshape(nz, ny, nx, 3),
                np.fromfile("%s.%d.grad" % (d / name, k), np.uint8).reshape(nz, ny, nx, 3))
    on, err_on = run(exe, [spec, "48", "48", "1", "on", seq], "on", d)
    off, err_off = run(exe, [spec, "48", "48", "1", "off", seq], "off", d)
    assert len(on) == len(off) == 5 and "ERROR" not in err_on and "ERROR" not in err_off, (err_on, err_off)
    assert max(f.max() for f in on) > 0.05
    for k, (a, b) in enumerate(((0, 1), (0, 1), (0, 1), (1, 2), (1, 2))):
        frac = k in (1, 2, 3)
        mixed = T.blend(steps[a][0], steps[a][1], steps[b][0], steps[b][1], np.float32(0.37))
        want_off = mixed if frac else steps[a]
        want_on = V.derive(O, np.ascontiguousarray(mixed[0][..., 0]), "u8", 1, 0) if frac else steps[a]
        for name, want in (("off", want_off), ("on", want_on)):
            got = shown(name, k)
            same(got[0], want[0], "%s, draw %d: data" % (name, k))
            same(got[1], want[1], "%s, draw %d: normals" % (name, k))
        assert np.array_equal(on[k], off[k]) == (not frac), "draw %d" % k
    assert np.array_equal(on[1], on[2]) and not np.array_equal(on[1], on[3])
    # A full ring: the series keeps two of its four steps resident, and the steps 2 and 3 go up into the slots the ring grew by
    # after the first fraction.  Every later blend and derived step then takes its slot by the ring's turn, which must never
    # be the slot of step 1 or 2, which the fractions after it blend (step 3 may go: nothing here blends it): no fraction is
    # refused, each shows the derivatives of its blend
    steps4 = steps + [V.series_step(O, V.scalar(3, dims), "u8")]
    data3, nrm3 = steps4[3]
    data3.tofile(str(d / "s.3.vgh"))
    nrm3.tofile(str(d / "s.3.nrm"))
    spec4 = "vgh:%s:%d:%d:%d:4:%s:2" % (d / "s", nx, ny, nz, d / "table.rgba")
    plan = ((1, 0), (0, 0), (0, 0.37), (2, 0), (3, 0), (1, 0.37), (1, 0.5), (1, 0.6), (1, 0.7))
    full, err_full = run(exe, [spec4, "48", "48", "1", "on", ",".join("%d:%g" % p for p in plan)], "full", d)
    assert len(full) == len(plan) and "ERROR" not in err_full, err_full
    for k, (t, f) in enumerate(plan):
        want = steps4[t]
        if f:
            mixed = T.blend(steps4[t][0], steps4[t][1], steps4[t + 1][0], steps4[t + 1][1], np.float32(f))
            want = V.derive(O, np.ascontiguousarray(mixed[0][..., 0]), "u8", 1, 0)
        got = shown("full", k)
        same(got[0], want[0], "full ring, draw %d: data" % k)
        same(got[1], want[1], "full ring, draw %d: normals" % k)
    # with derivatives off, on the scalar series tblend_main plays: its frames
    steps1 = [np.ascontiguousarray(T.step("u8", s)[0][..., 0]) for s in (1, 2, 3)]
    e = tmp_path / "scalar"
    e.mkdir()
    trex = write_series(str(e), steps1, shape=(32, 32, 32), tstart=0, cache=3)
    seq1 = "0:0,0:0.3,0:0.7,1:0.7"
    ref, _ = run(tblend, ["frac", trex, "48", "48", "1", seq1], "ref", e)
    got, err = run(exe, [trex, "48", "48", "1", "off", seq1], "off", e)
    assert len(ref) == len(got) == 4 and not np.array_equal(ref[0], ref[1]) and "ERROR" not in err
    for k in range(4):
        assert np.array_equal(got[k], ref[k]), "draw %d" % k
    # ... and on: a scalar series has no G and H to derive -- said once per blend, and the frames show the blend
    got, err = run(exe, [trex, "48", "48", "1", "on", seq1 + ",1:0.7"], "on", e)
    assert err.count("setTimeFractionDerivatives") == 3 and err.count("nelts 1") == 3, err
    for k in range(4):
        assert np.array_equal(got[k], ref[k]), "draw %d" % k
    assert np.array_equal(got[4], ref[3])
