"""Merged fields of a step (smk.h smk_merge_timestep, smk_upload_timestep_fields_device): the step made inside the ring must
be, bit for bit, the step a FRESH context holds after it uploaded what the recipe "Merged fields of a blend" (INTEGRATION.md
5) makes of the same fields with the existing device entries (smk_merge_fields_device, smk_merge_fields_f32_device,
smk_quantize_u16_device) in the same test -- voxels and normals as smk_download_timestep returns them, frames on the gather
and the slice-ring kernel, the step histogram.  Where the fields are finite and their summed gradient is not zero everywhere
the arrays are also the restatement's (tests/_step_merge_ref.py, qualified by tests/test_step_merge_cpu.py).  Volumes are
37 x 13 x 11 and 70 x 21 x 19 voxels, the kernels' tile sizes and a thin 5 x 190 x 175."""
import os
import subprocess

import numpy as np
import pytest

import _step_merge_ref as M
import _tblend_ref as T
from _gpu_mem import dev_ptr as dev, field_ptrs, out_buffer, stream_arg
from _step_gpu import MODE, RAN, Undisturbed, fresh_download, same_bits as same, scene_context, series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.37


def recipe(R, F):
    """what the recipe's device entries make of the fields F [z][y][x][nf] (u8, u16 or f32) for a ring of F's type:
    (data [z][y][x][nf + 1], normals) as host arrays, made on the device through context R"""
    F = np.ascontiguousarray(F)
    nz, ny, nx, nf = F.shape
    dims, n = (nx, ny, nz), nx * ny * nz
    nrm = out_buffer(n * 3, np.uint8)                       # (the entries run on the context's stream)
    if F.dtype == np.uint8:
        pf, keep = dev(F)
        out = out_buffer(n * (nf + 1), np.uint8)
        R.merge_fields_device(pf, nf, dims, out.data_ptr(), nrm.data_ptr())
        data = out.cpu().numpy().reshape(nz, ny, nx, nf + 1)
    else:
        pf, keep = dev(F.astype(np.float32))                # u16: F = (float)v, unscaled
        out = out_buffer(n * (nf + 1), np.float32)
        R.merge_fields_f32_device(pf, nf, dims, out.data_ptr(), nrm.data_ptr())
        data = out.cpu().numpy().reshape(nz, ny, nx, nf + 1)
        if F.dtype == np.uint16:
            g = out.view(n, nf + 1)[:, nf].contiguous()     # G, a strided device copy
            q = out_buffer(n * 2, np.uint8)                 # (it waits for that copy too)
            R.quantize_u16_device(g.data_ptr(), n, q.data_ptr())
            gq = q.cpu().numpy().view(np.uint16).reshape(nz, ny, nx, 1)
            data = np.ascontiguousarray(np.concatenate([F, gq], -1))
    return data, nrm.cpu().numpy().reshape(nz, ny, nx, 3)


def recipe_download(factory, R, F, normals=True):
    return fresh_download(factory, *recipe(R, F), MODE, normals=normals)


def both_forms(factory, F, normals=True, cap=3):
    """(the download of smk_merge_timestep's output, of smk_upload_timestep_fields_device's, the recipe's) for the fields F;
    the source step -- the fields, a last channel and normals that are not theirs -- must be unchanged afterwards"""
    nz, ny, nx, nf = F.shape
    sdata, snrm = M.source_step(F)
    src = M.downloaded(sdata, snrm, normals)
    R = series(factory, ((sdata, snrm if normals else None),), cap=cap, dm=MODE)
    try:
        R.merge_timestep(0, 1)
        assert R.timesteps() == (0, [0, 1])                 # (a merged step does not become current)
        got = R.download_timestep(1)
        ptrs, keep = field_ptrs(F)
        R.upload_timestep_fields_device(2, ptrs, M.CODE[M.RING_OF[F.dtype]], (nx, ny, nz))
        assert R.timesteps() == (0, [0, 1, 2])
        got2 = R.download_timestep(2)
        back = R.download_timestep(0)
        same(back[0], src[0], "the source, afterwards")
        same(back[1], src[1], "the source's normals, afterwards")
        stored = np.ascontiguousarray(back[0][..., :nf])    # the fields as the recipe reads them back and de-interleaves them
        same(stored, F, "the stored fields")
        want = recipe_download(factory, R, stored, normals=normals)
    finally:
        R.close()
    return got, got2, want


def check(got, got2, want, what):
    same(got[0], want[0], what + ": data")
    same(got[1], want[1], what + ": normals")
    same(got2[0], want[0], what + ", fields form: data")
    same(got2[1], want[1], what + ", fields form: normals")


# ---- 1. both forms in every ring type

@pytest.mark.parametrize("normals", (True, False), ids=("normals", "no-normals"))
@pytest.mark.parametrize("dims", M.DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("ring, nf", M.CASES)
def test_both_forms_equal_the_recipe_and_the_restatement(gpu_renderer_factory, O, ring, nf, dims, normals):
    F = M.fields(ring, nf, dims)
    got, got2, want = both_forms(gpu_renderer_factory, F, normals)
    check(got, got2, want, "%s nf %d" % (ring, nf))
    ref = M.downloaded(*M.merge(O, F), normals=normals)
    same(got[0], ref[0], "data against the restatement")
    same(got[1], ref[1], "normals against the restatement")
    assert got[0][..., nf].any() and ((got[1] != 128).any() == normals)
    if not normals:
        assert (got[1] == 128).all()


# ---- 2. edges of the kernels' tiles and of pass 1's grid

@pytest.mark.parametrize("ring", M.RINGS)
def test_tile_edges_with_the_maximum_in_the_last_tile(gpu_renderer_factory, O, ring):
    for dims in M.tile_shapes(ring):
        F, at = M.planted_last(ring, 2, dims)
        got, got2, want = both_forms(gpu_renderer_factory, F)
        check(got, got2, want, "%s %s" % (ring, dims))
        ref = M.downloaded(*M.merge(O, F))
        same(got[0], ref[0], "%s %s: data against the restatement" % (ring, dims))
        same(got[1], ref[1], "%s %s: normals against the restatement" % (ring, dims))


@pytest.mark.parametrize("ring", M.RINGS)
def test_more_tiles_than_workgroups_of_pass_1(gpu_renderer_factory, O, ring):
    """the planted maximum lies in a tile that only a workgroup's second turn reaches (tests/test_step_merge_cpu.py)"""
    F = M.thin_fields(ring)
    got, got2, want = both_forms(gpu_renderer_factory, F)
    check(got, got2, want, "thin " + ring)
    ref = M.downloaded(*M.merge(O, F))
    same(got[0], ref[0], "data against the restatement")
    same(got[1], ref[1], "normals against the restatement")


# ---- 3. degenerate and non-finite inputs, against the device recipe

def degenerate():
    rng = np.random.default_rng(11)
    out = []
    for ring in M.RINGS:
        out.append(("constant-" + ring, np.full((6, 5, 7, 2), 93, M.NP[ring])))
        out.append(("3x3x3-" + ring, M.noise(ring, 2, (3, 3, 3))))
    f0 = rng.integers(0, 256, (7, 6, 9), dtype=np.uint8)
    out.append(("cancel-u8", np.ascontiguousarray(np.stack([f0, 255 - f0], -1))))
    for nf in (2, 3):
        F = M.fields("f32", nf, (9, 7, 6)).copy()
        F[2, 3, 4, 0], F[3, 2, 6, 1], F[2, 4, 2, nf - 1] = np.nan, np.inf, np.float32(-0.0)
        F.view(np.uint32)[4, 3, 3, 0] = 0x7fc12345           # a NaN with a payload
        out.append(("nonfinite-f32-nf%d" % nf, F))
    return out


@pytest.mark.parametrize("name, F", degenerate(), ids=[d[0] for d in degenerate()])
def test_degenerate_and_nonfinite_inputs_equal_the_recipe(gpu_renderer_factory, name, F):
    got, got2, want = both_forms(gpu_renderer_factory, F)
    check(got, got2, want, name)
    nf = F.shape[-1]
    if name.startswith(("constant", "cancel")):             # a maximum of 0: G is 0 everywhere, every normal the zero vector's
        assert not got[0][..., nf].any() and (got[1] == 128).all()
    if name.startswith("nonfinite"):
        assert (got[0][..., nf] > 0).any() and np.isfinite(got[0][..., nf]).all()
        assert (got[1][2, 3, 3:6:2] == 128).all()           # the x neighbours of the NaN: a non-finite gradient


# ---- 4. a merged step is a step

FRAMES = (("u8", 2, 1), ("u8", 2, 2), ("u16", 2, 1), ("f32", 2, 1), ("f32", 3, 1))


@pytest.mark.parametrize("ring, nf, kernel", FRAMES, ids=["%s-nf%d-%s" % (r, n, {1: "gather", 2: "slice-ring"}[k]) for r, n, k in FRAMES])
def test_a_merged_step_renders_and_counts_like_the_recipes_upload(gpu_renderer_factory, ring, nf, kernel):
    from _scenes import push_scene
    dims = M.DIMS[1]
    F = M.fields(ring, nf, dims)
    sdata, snrm = M.source_step(F)
    opts = (("kernel", kernel), ("bricks", 1))
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(3)
        push_scene(R, T.scene(sdata, snrm))
        for k, v in opts:
            R.set_option(k, v)
        before = R.render()
        R.merge_timestep(0, 1)
        R.select_timestep(1)
        got = R.render()
        assert R.last_frame_info()[0] == RAN[kernel]
        flags = R.brick_flags()[0]
        counts = R.hist2d_step(1)
        data, nrm = recipe(R, F)
        assert R.stat("slab_failures") == 0
    finally:
        R.close()
    Fr = gpu_renderer_factory()
    try:
        push_scene(Fr, T.scene(data, nrm))
        for k, v in opts:
            Fr.set_option(k, v)
        want = Fr.render()
        assert Fr.last_frame_info()[0] == RAN[kernel]
        wflags = Fr.brick_flags()[0]
        wcounts = Fr.hist2d_step()
    finally:
        Fr.close()
    assert want[..., 3].max() > 0.05 and not np.array_equal(before, want)
    assert np.array_equal(flags, wflags), "brick flags"
    assert np.array_equal(counts, wcounts), "step histogram"
    assert np.array_equal(got, want), "frame: max diff %g" % np.abs(got - want).max()


# ---- 5. slots, ordering, refusals

def test_in_place_overwrite_of_a_cached_output_that_is_current(gpu_renderer_factory, O):
    dims = M.SMALL
    Fa, Fb = M.fields("u8", 2, dims, 0), M.fields("u8", 2, dims, 1)
    a, b = M.source_step(Fa), M.source_step(Fb, 6)
    wa, wb = M.downloaded(*M.merge(O, Fa)), M.downloaded(*M.merge(O, Fb))
    R = series(gpu_renderer_factory, (a, b), cap=3, dm=MODE)
    try:
        R.merge_timestep(1, 5)
        assert R.timesteps() == (0, [0, 1, 5])
        R.merge_timestep(1, 6)                              # no empty slot: the one behind the last written, past the
        assert R.timesteps() == (0, [0, 1, 6])              # current step's and the source's
        same(R.download_timestep(6)[0], wb[0], "capacity 3")
        R.merge_timestep(0, 6)                              # a cached output is overwritten in place
        assert R.timesteps() == (0, [0, 1, 6])
        same(R.download_timestep(6)[0], wa[0], "in place")
        R.select_timestep(6)
        R.merge_timestep(1, 6)                              # ... the current step too
        assert R.timesteps() == (6, [0, 1, 6])
        same(R.download_timestep()[0], wb[0], "the current step overwritten")
        same(R.download_timestep()[1], wb[1], "the current step overwritten: normals")
        ptrs, keep = field_ptrs(Fa)
        R.upload_timestep_fields_device(6, ptrs, 0, dims)   # ... and by the fields form
        assert R.timesteps() == (6, [0, 1, 6])
        same(R.download_timestep()[0], wa[0], "the current step overwritten by the fields form")
    finally:
        R.close()


def test_merge_on_a_side_stream_behind_a_blend_and_a_source_overwritten(gpu_renderer_factory):
    import torch
    dims = M.SMALL
    nx, ny, nz = dims
    for ring, nf in (("u8", 2), ("f32", 3)):
        Fa, Fb, Fc = (M.fields(ring, nf, dims, s) for s in (0, 1, 2))
        a, b, c = M.source_step(Fa), M.source_step(Fb, 6), M.source_step(Fc, 7)
        side, up = torch.cuda.Stream(), torch.cuda.Stream()
        pc, kc = dev(c[0])
        pg, kg = dev(c[1])
        work = out_buffer(1 << 22, np.float32)
        R = series(gpu_renderer_factory, (a, b), cap=4, dm=MODE)
        try:
            torch.cuda.synchronize()                        # nothing is in flight when the two streams start
            with torch.cuda.stream(side):                   # work in front of the blend: nothing behind it has started yet
                for _ in range(24):
                    work.add_(1)
            R.blend_timesteps(0, 1, W, 2, stream=stream_arg(side))
            R.merge_timestep(2, 3, stream=stream_arg(side))  # directly behind the blend, no host wait
            R.upload_timestep_device(2, pc, dims, nf + 1, M.CODE[ring], pg, dmode=MODE[nf + 1],
                                     stream=stream_arg(up))  # the source slot overwritten: behind the merge's reads
            torch.cuda.synchronize()                        # both streams have ended: the host forms below read their results
            got = R.download_timestep(3)
            same(R.download_timestep(2)[0], M.downloaded(*c)[0], "the new step 2")
            R.blend_timesteps(0, 1, W, 2)                   # the synchronous results: the blend again, and the recipe of its fields
            mixed = R.download_timestep(2)
            same(mixed[0], M.downloaded(*T.blend(a[0], a[1], b[0], b[1], np.float32(W)))[0], "the blend")
            want = recipe_download(gpu_renderer_factory, R, np.ascontiguousarray(mixed[0][..., :nf]))
        finally:
            R.close()
        same(got[0], want[0], ring + ": data")
        same(got[1], want[1], ring + ": normals")
        assert not np.array_equal(got[0][..., nf], mixed[0][..., nf]), "vacuous: the blend of G is G of the blend"


def test_refusals(gpu_renderer_factory, smk, O):
    dims = M.SMALL
    nx, ny, nz = dims
    F = M.fields("u8", 2, dims)
    a = M.source_step(F)
    b = M.source_step(M.fields("u8", 2, dims, 1), 6)
    buf = out_buffer(nx * ny * nz * 4 + 64, np.uint8)
    p0, p1 = buf.data_ptr(), buf.data_ptr() + nx * ny * nz
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match="smk_merge_timestep: no volume"):
            R.merge_timestep(0, 1)
        with pytest.raises(smk.SmkError, match="smk_upload_timestep_fields_device: no volume"):
            R.upload_timestep_fields_device(1, [p0, p1], 0, dims)
    finally:
        R.close()
    sca = T.scene(*a)
    fsize = tuple(float(f) for f in sca.fsize)
    R = scene_context(gpu_renderer_factory, sca, cap=2)
    try:
        R.upload_timestep(1, b[0], b[1], fsize=fsize, dmode="VGH")         # (the scene's data mode; the merge does not look at it)
        with Undisturbed(R):                                # a refused call changes nothing: frames, flags, steps
            for args, why in (((99, 5), r"99 \(the source\) is not cached"), ((-1, 5), "is not cached"), ((0, -1), ">= 0"),
                              ((1, 1), "in-place"), ((1, 5), "holds 2 steps.*here 3")):
                with pytest.raises(smk.SmkError, match="smk_merge_timestep: .*" + why):
                    R.merge_timestep(*args)
            for args, why in (((5, None, 0, dims), "d_fields is NULL"), ((5, [p0, None], 0, dims), r"d_fields\[1\] is NULL"),
                              ((5, [p0], 0, dims), "1 fields for a series of nelts 3"),
                              ((5, [p0, p1, p0], 0, dims), "3 fields for a series of nelts 3"),
                              ((5, [p0, p1], 1, dims), r"field_dtype 1 is not the ring's type \(0\)"),
                              ((5, [p0, p1], 7, dims), "field_dtype 7"),
                              ((5, [p0, p1], 0, (nx, ny + 1, nz)), "differ from the series'"), ((-3, [p0, p1], 0, dims), ">= 0")):
                with pytest.raises(smk.SmkError, match="smk_upload_timestep_fields_device: .*" + why):
                    R.upload_timestep_fields_device(*args)
        assert R.timesteps() == (0, [0, 1])
        R.merge_timestep(0, 5)                              # the only slot that is neither the source's nor current: step 1's
        assert R.timesteps() == (0, [0, 5])
        same(R.download_timestep(5)[0], M.downloaded(*M.merge(O, F))[0], "capacity 2")
    finally:
        R.close()
    # alignment of a field below its element: 16-bit and float rings
    for ring, off, size in (("u16", 1, 2), ("f32", 2, 4)):
        st = M.source_step(M.fields(ring, 2, dims))
        R = scene_context(gpu_renderer_factory, T.scene(*st), cap=3)
        try:
            with Undisturbed(R):
                with pytest.raises(smk.SmkError, match=r"d_fields\[1\] is not aligned to its %d-byte" % size):
                    R.upload_timestep_fields_device(1, [p0, p0 + off], M.CODE[ring], dims)
            assert R.timesteps() == (0, [0])
        finally:
            R.close()
    # a series of one channel; a sharded context
    one = np.ascontiguousarray(a[0][..., :1])
    R = scene_context(gpu_renderer_factory, T.scene(one, a[1]), cap=3)
    try:
        frame = R.render()                                  # (a 1-D table flags no bricks: Undisturbed does not apply)
        assert frame[..., 3].max() > 0.05
        with pytest.raises(smk.SmkError, match="smk_merge_timestep: the series has nelts 1"):
            R.merge_timestep(0, 1)
        with pytest.raises(smk.SmkError, match="smk_upload_timestep_fields_device: the series has nelts 1"):
            R.upload_timestep_fields_device(1, [p0], 0, dims)
        assert R.timesteps() == (0, [0]) and np.array_equal(R.render(), frame)
        same(R.download_timestep()[0], one, "after the refusals")
        same(R.download_timestep()[1], a[1], "the normals after the refusals")
    finally:
        R.close()
    R = scene_context(gpu_renderer_factory, sca, cap=3, shard=(0, 2))
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match="smk_merge_timestep: a sharded context.*1 voxel beyond region \\+ halo.*whole volume's maximum"):
                R.merge_timestep(0, 1)
            with pytest.raises(smk.SmkError, match="smk_upload_timestep_fields_device: a sharded context"):
                R.upload_timestep_fields_device(1, [p0, p1], 0, dims)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    # a cache of one step -- a context that never asked for a series -- holds the current step and no other: no slot
    R = scene_context(gpu_renderer_factory, sca)
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match="smk_upload_timestep_fields_device: time step 5: the cache holds one step, the current one"):
                R.upload_timestep_fields_device(5, [p0, p1], 0, dims)
            with pytest.raises(smk.SmkError, match="smk_merge_timestep: the cache holds 1 steps.*here 2"):
                R.merge_timestep(0, 5)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    # a volume thinner than 3 voxels has no interior voxel (smk_merge_fields_device refuses it too)
    thin = (np.ascontiguousarray(a[0][:2]), np.ascontiguousarray(a[1][:2]))
    R = scene_context(gpu_renderer_factory, T.scene(*thin), cap=3)
    try:
        with Undisturbed(R, visible=False):
            with pytest.raises(smk.SmkError, match="smk_merge_timestep: a 37x13x2 volume has no interior voxel"):
                R.merge_timestep(0, 1)
            with pytest.raises(smk.SmkError, match="smk_upload_timestep_fields_device: a 37x13x2 volume has no interior voxel"):
                R.upload_timestep_fields_device(1, [p0, p1], 0, (nx, ny, 2))
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    assert not buf.any()


# ---- 6. the host adapter

def test_host_adapter_shows_the_merged_fields_of_a_blend(tmp_path, O):
    """tests/host/merge_main drives HipVolumeRenderable::setTimeFraction + setTimeFractionDerivatives over a 3-step two-field
    u8 series (GDM_V2G): with derivatives on the step a fractional frame shows is the restatement's merge of the blended
    fields; with them off it is the plain blend"""
    exe = os.path.join(ROOT, "tests", "host", "merge_main")
    assert os.path.exists(exe), "%s is not built: __graft_entry__.build() builds it" % exe
    dims = M.SMALL
    nx, ny, nz = dims
    steps = [M.merge(O, M.fields("u8", 2, dims, s)) for s in (0, 1, 2)]    # what the host prepared with mergeMV -addG
    d = tmp_path / "mf"
    d.mkdir()
    for t, (data, nrm) in enumerate(steps):
        data.tofile(str(d / ("s.%d.mf" % t)))
        nrm.tofile(str(d / ("s.%d.nrm" % t)))
    tex = np.zeros((256, 256, 4), np.uint8)
    tex[..., 0] = np.arange(256, dtype=np.uint8)[None, :]
    tex[..., 1] = 255 - np.arange(256, dtype=np.uint8)[None, :]
    tex[..., 2] = 90
    tex[..., 3] = 60
    tex.tofile(str(d / "table.rgba"))
    spec = "%s:%d:%d:%d:3:3:%s" % (d / "s", nx, ny, nz, d / "table.rgba")
    seq = "0:0,0:0.37,0:0.37,1:0.37,1:0.6,1:0"

    def run(onoff, name):
        p = subprocess.run([exe, spec, "48", "48", "1", onoff, seq, str(d / name)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        n = sum(line.startswith("frame ") for line in p.stdout.splitlines())
        return [np.fromfile("%s.%d.f32" % (d / name, k), np.float32) for k in range(n)], p.stderr

    def shown(name, k):
        return (np.fromfile("%s.%d.data" % (d / name, k), np.uint8).reshape(nz, ny, nx, 3),
                np.fromfile("%s.%d.grad" % (d / name, k), np.uint8).reshape(nz, ny, nx, 3))
    on, err_on = run("on", "on")
    off, err_off = run("off", "off")
    assert len(on) == len(off) == 6 and "ERROR" not in err_on and "ERROR" not in err_off, (err_on, err_off)
    assert max(f.max() for f in on) > 0.05
    for k, (t, f) in enumerate(((0, 0), (0, .37), (0, .37), (1, .37), (1, .6), (1, 0))):
        mixed = T.blend(steps[t][0], steps[t][1], steps[t + 1][0], steps[t + 1][1], np.float32(f)) if f else steps[t]
        want_on = M.merge(O, np.ascontiguousarray(mixed[0][..., :2])) if f else steps[t]
        for name, want in (("off", mixed), ("on", want_on)):
            got = shown(name, k)
            same(got[0], want[0], "%s, draw %d: data" % (name, k))
            same(got[1], want[1], "%s, draw %d: normals" % (name, k))
        if f:
            assert not np.array_equal(want_on[0], mixed[0]) and not np.array_equal(want_on[1], mixed[1]), "vacuous"
        if not f:                                           # (a whole step is the same frame either way)
            assert np.array_equal(on[k], off[k]), "draw %d" % k
    assert np.array_equal(on[1], on[2]) and not np.array_equal(on[1], on[3]) and not np.array_equal(off[0], off[1])
