"""Merged fields with H and blurred normals (smk.h smk_merge_timestep_h, smk_upload_timestep_fields_h_device,
smk_merge_fields_h_device, smk_merge_fields_h_f32_device): the step made inside the ring must be, bit for bit, the step that
smk_upload_timestep_device packs from what the preparation entries (and, for a u16 ring, smk_quantize_u16_device) make of the
same fields in the same test -- voxels and normals as smk_download_timestep returns them, frames on the gather and the
slice-ring kernel, the step histogram -- and the restatement's (tests/_step_merge_h_ref.py, qualified by
tests/test_step_merge_h_cpu.py).  Volumes are a few tiles of 32 x 8 x 8 voxels, 3 x 3 x 3 and a thin 5 x 380 x 350."""
import os
import subprocess

import numpy as np
import pytest

import _step_merge_h_ref as H
import _step_merge_ref as M
import _tblend_ref as T
from _gpu_mem import dev_ptr as dev, field_ptrs, out_buffer, stream_arg
from _step_gpu import RAN, Undisturbed, context, same_bits as same, scene_context

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 0.37
WITH_H = (("u8", 1), ("u8", 2), ("u16", 1), ("f32", 1), ("f32", 2))       # every (add_h, blur, compat)
BLUR_ONLY = (("u8", 3), ("u16", 2), ("f32", 3))                           # a voxel has no room for H: add_h 0


def mode(data, add_h):
    """the data mode of a step of fields, G and (add_h) H"""
    return H.MODE[(data.shape[-1] - 1 - add_h, add_h)]


def recipe(R, F, add_h, compat, blur):
    """what the preparation entries make of the fields F [z][y][x][nf] (u8, u16 or f32) for a ring of F's type:
    (data [z][y][x][nf + 1 + add_h], normals) as host arrays, made on the device through context R"""
    F = np.ascontiguousarray(F)
    nz, ny, nx, nf = F.shape
    dims, n, ne = (nx, ny, nz), nx * ny * nz, nf + 1 + add_h
    nrm = out_buffer(n * 3, np.uint8)                       # (the entries run on the context's stream)
    if F.dtype == np.uint8:
        pf, keep = dev(F)
        out = out_buffer(n * ne, np.uint8)
        R.merge_fields_h_device(pf, nf, dims, out.data_ptr(), nrm.data_ptr(), add_h, compat, blur)
        data = out.cpu().numpy().reshape(nz, ny, nx, ne)
    else:
        pf, keep = dev(F.astype(np.float32))                # u16: F = (float)v, unscaled
        out = out_buffer(n * ne, np.float32)
        R.merge_fields_h_f32_device(pf, nf, dims, out.data_ptr(), nrm.data_ptr(), add_h, compat, blur)
        data = out.cpu().numpy().reshape(nz, ny, nx, ne)
        if F.dtype == np.uint16:
            chans = [F]
            for k in range(nf, ne):                         # G, then H: strided device copies, quantised
                g = out.view(n, ne)[:, k].contiguous()
                q = out_buffer(n * 2, np.uint8)             # (it waits for that copy too)
                R.quantize_u16_device(g.data_ptr(), n, q.data_ptr())
                chans.append(q.cpu().numpy().view(np.uint16).reshape(nz, ny, nx, 1))
            data = np.ascontiguousarray(np.concatenate(chans, -1))
    return data, nrm.cpu().numpy().reshape(nz, ny, nx, 3)


def upload_recipe(R, step, F, add_h, compat, blur, normals=True):
    """the recipe's arrays uploaded as step `step` of R from device memory (smk_upload_timestep_device), downloaded"""
    nz, ny, nx, nf = F.shape
    data, nrm = recipe(R, F, add_h, compat, blur)
    pd, k0 = dev(data)
    pn, k1 = dev(nrm)
    R.upload_timestep_device(step, pd, (nx, ny, nz), data.shape[-1], H.CODE[H.RING_OF[F.dtype]], pn if normals else None,
                             dmode=H.MODE[(nf, add_h)])
    return R.download_timestep(step)


def both_forms(factory, F, add_h, compat, blur, normals=True):
    """(the download of smk_merge_timestep_h's output, of smk_upload_timestep_fields_h_device's, the recipe's) for the fields
    F; the source step -- the fields, last channels and normals that are not theirs -- must be unchanged afterwards"""
    nz, ny, nx, nf = F.shape
    sdata, snrm = H.source_step(F, add_h)
    src = M.downloaded(sdata, snrm, normals)
    R = context(factory, sdata, snrm if normals else None, cap=4, dm=mode(sdata, add_h))
    try:
        R.merge_timestep_h(0, 1, add_h, compat, blur)
        assert R.timesteps() == (0, [0, 1])                 # (a merged step does not become current)
        got = R.download_timestep(1)
        ptrs, keep = field_ptrs(F)
        R.upload_timestep_fields_h_device(2, ptrs, H.CODE[H.RING_OF[F.dtype]], (nx, ny, nz), add_h, compat, blur)
        assert R.timesteps() == (0, [0, 1, 2])
        got2 = R.download_timestep(2)
        back = R.download_timestep(0)
        same(back[0], src[0], "the source, afterwards")
        same(back[1], src[1], "the source's normals, afterwards")
        want = upload_recipe(R, 3, F, add_h, compat, blur, normals)
    finally:
        R.close()
    return got, got2, want


def check(F, got, got2, want, add_h, compat, blur, normals, what):
    same(got[0], want[0], what + ": data")
    same(got[1], want[1], what + ": normals")
    same(got2[0], want[0], what + ", fields form: data")
    same(got2[1], want[1], what + ", fields form: normals")
    ref = H.downloaded(*H.merge_h(F, add_h, compat, blur), normals=normals)
    same(got[0], ref[0], what + ": data against the restatement")
    same(got[1], ref[1], what + ": normals against the restatement")


def tag(add_h, compat, blur):
    return "add_h %d compat %d blur %d" % (add_h, compat, blur)


# ---- 1. both forms in every ring type, at the tile's edges

@pytest.mark.parametrize("ring, nf", WITH_H + BLUR_ONLY, ids=lambda v: str(v))
def test_both_forms_equal_the_recipe_and_the_restatement(gpu_renderer_factory, ring, nf):
    flags = [f for f in H.FLAGS if (ring, nf) in WITH_H or not f[0]]
    for i, (add_h, blur, compat) in enumerate(flags):
        dims = H.SHAPES[(i + nf) % len(H.SHAPES)]
        normals = i % 4 != 3
        F = H.fields(ring, nf, dims)
        got, got2, want = both_forms(gpu_renderer_factory, F, add_h, compat, blur, normals)
        what = "%s nf %d %s %s" % (ring, nf, dims, tag(add_h, compat, blur))
        check(F, got, got2, want, add_h, compat, blur, normals, what)
        assert got[0][..., nf].any() and ((got[1] != 128).any() == normals), what
        if add_h:
            assert len(np.unique(got[0][..., nf + 1])) > 20, what


@pytest.mark.parametrize("ring", H.RINGS)
def test_every_shape_with_h_and_blur(gpu_renderer_factory, ring):
    for k, dims in enumerate(H.SHAPES):
        F = H.fields(ring, 1, dims)
        got, got2, want = both_forms(gpu_renderer_factory, F, 1, k & 1, 1)
        check(F, got, got2, want, 1, k & 1, 1, True, "%s %s" % (ring, dims))


# ---- 2. the old twins' bits with add_h = blur = 0

@pytest.mark.parametrize("ring, nf", (("u8", 3), ("u16", 2), ("f32", 3), ("f32", 1)))
def test_without_h_and_blur_the_old_entries_bits(gpu_renderer_factory, ring, nf):
    dims = H.SHAPES[1]
    nx, ny, nz = dims
    F = H.fields(ring, nf, dims)
    sdata, snrm = H.source_step(F, 0)
    R = context(gpu_renderer_factory, sdata, snrm, cap=5, dm=mode(sdata, 0))
    try:
        R.merge_timestep(0, 1)
        R.merge_timestep_h(0, 2, 0, 1, 0)
        ptrs, keep = field_ptrs(F)
        R.upload_timestep_fields_device(3, ptrs, H.CODE[ring], dims)
        R.upload_timestep_fields_h_device(4, ptrs, H.CODE[ring], dims, 0, 0, 0)
        a, b, c, d = (R.download_timestep(t) for t in (1, 2, 3, 4))
        for x, what in ((b, "merge_timestep_h"), (c, "the old fields form"), (d, "the fields form")):
            same(x[0], a[0], what + ": data")
            same(x[1], a[1], what + ": normals")
        assert a[0][..., nf].any() and (a[1] != 128).any()
        if ring != "u16":                                   # the preparation entries, array for array
            n = nx * ny * nz
            Fd = F if ring == "u8" else F.astype(np.float32)
            pf, k0 = dev(Fd)
            outs = [out_buffer(n * (nf + 1), Fd.dtype) for _ in range(2)]
            nrms = [out_buffer(n * 3, np.uint8) for _ in range(2)]
            old, new = (R.merge_fields_device, R.merge_fields_h_device) if ring == "u8" else (R.merge_fields_f32_device, R.merge_fields_h_f32_device)
            old(pf, nf, dims, outs[0].data_ptr(), nrms[0].data_ptr())
            new(pf, nf, dims, outs[1].data_ptr(), nrms[1].data_ptr(), 0, 1, 0)
            same(outs[1].cpu().numpy(), outs[0].cpu().numpy(), "the preparation entry: data")
            same(nrms[1].cpu().numpy(), nrms[0].cpu().numpy(), "the preparation entry: normals")
            assert outs[0].any() and (nrms[0] != 128).any()
    finally:
        R.close()


# ---- 3. degenerate and non-finite inputs

def all_negative(ring):
    """one field of 4 x 3 x 3 voxels, constant in y and z, whose two interior voxels both have hs < 0: the neighbours' summed
    gradients are 0 on the border, so S = (100, 0, 0) and (-150, 0, 0) give h[0] = -150 - 0 and 0 - 100.  max H stays below 0"""
    v = np.broadcast_to(np.array([0, 200, 100, 50], np.uint8), (3, 3, 4))
    return np.ascontiguousarray(M.as_type(v, ring)[..., None])


def degenerate():
    out = []
    for ring in H.RINGS:
        out.append(("constant-" + ring, np.full((6, 5, 7, 1), 93, H.NP[ring]), 1))
        out.append(("3x3x3-" + ring, M.noise(ring, 1, H.TINY), 1))
        out.append(("negative-" + ring, all_negative(ring), 0))
    F = M.fields("f32", 2, (9, 7, 6)).copy()
    F[2, 3, 4, 0], F[3, 2, 6, 1], F[2, 4, 2, 1], F[4, 4, 4, 0] = np.nan, np.inf, np.float32(-0.0), -np.inf
    F.view(np.uint32)[4, 3, 3, 0] = 0x7fc12345               # a NaN with a payload
    out.append(("nonfinite-f32", F, 1))
    return out


@pytest.mark.parametrize("name, F, compat", degenerate(), ids=[d[0] for d in degenerate()])
def test_degenerate_and_nonfinite_inputs(gpu_renderer_factory, name, F, compat):
    nf = F.shape[-1]
    for blur in (0, 1):
        got, got2, want = both_forms(gpu_renderer_factory, F, 1, compat, blur)
        check(F, got, got2, want, 1, compat, blur, True, name)
        Hc = got[0][..., nf + 1]
        if name.startswith("constant"):                     # a maximum of 0: G is 0, every interior H is NaN's 0, the border's 85
            assert not got[0][..., nf].any() and (got[1] == 128).all() and not Hc[1:-1, 1:-1, 1:-1].any() and Hc[0].all()
        if name.startswith("negative"):
            hs = H.second_derivative(H.summed(F.astype(np.float32)), 0)[1:-1, 1:-1, 1:-1]
            assert hs.size == 2 and (hs < 0).all() and H.h_extremes(np.pad(hs, 1), H.RING_OF[F.dtype] != "u8")[1] < 0
            assert Hc[0].all() and Hc[1, 1, 2] != Hc[1, 1, 1], "the border's 0 scales against a negative max H; the two voxels differ"
        if name.startswith("nonfinite"):
            assert np.isfinite(Hc).all() and np.isfinite(got[0][..., nf]).all() and len(np.unique(Hc)) > 10


# ---- 4. more tiles than pass 1 has workgroups

@pytest.mark.parametrize("ring", H.RINGS)
def test_more_tiles_than_workgroups_of_pass_1(gpu_renderer_factory, ring):
    """the three extremes lie in tiles that only a workgroup's second turn reaches (tests/test_step_merge_h_cpu.py)"""
    F = H.thin_fields(ring)
    got, got2, want = both_forms(gpu_renderer_factory, F, 1, 1, 0)
    check(F, got, got2, want, 1, 1, 0, True, "thin " + ring)


# ---- 5. a merged step is a step

FRAMES = (("u8", 2, 1), ("u8", 2, 2), ("u16", 1, 1), ("f32", 2, 1))


@pytest.mark.parametrize("ring, nf, kernel", FRAMES, ids=["%s-nf%d-%s" % (r, n, {1: "gather", 2: "slice-ring"}[k]) for r, n, k in FRAMES])
def test_a_merged_step_renders_and_counts_like_the_recipes_upload(gpu_renderer_factory, ring, nf, kernel):
    from _scenes import push_scene
    dims = H.MAIN
    F = H.fields(ring, nf, dims)
    sdata, snrm = H.source_step(F, 1)
    opts = (("kernel", kernel), ("bricks", 1))
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(3)
        push_scene(R, T.scene(sdata, snrm))
        for k, v in opts:
            R.set_option(k, v)
        before = R.render()
        R.merge_timestep_h(0, 1, 1, 1, 1)
        R.select_timestep(1)
        got = R.render()
        assert R.last_frame_info()[0] == RAN[kernel]
        flags = R.brick_flags()[0]
        counts = R.hist2d_step(1)
        data, nrm = recipe(R, F, 1, 1, 1)
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


# ---- 6. slots, ordering, refusals

def test_in_place_overwrite_of_a_cached_output_that_is_current(gpu_renderer_factory):
    dims = M.SMALL
    Fa, Fb = H.fields("u8", 2, dims, 0), H.fields("u8", 2, dims, 1)
    a, b = H.source_step(Fa, 1), H.source_step(Fb, 1, 6)
    wa, wb = H.downloaded(*H.merge_h(Fa, 1, 1, 1)), H.downloaded(*H.merge_h(Fb, 1, 1, 1))
    R = context(gpu_renderer_factory, a[0], a[1], cap=3, dm=mode(a[0], 1))
    try:
        R.upload_timestep(1, b[0], b[1], dmode="V2GH")
        R.merge_timestep_h(1, 5, 1, 1, 1)
        assert R.timesteps() == (0, [0, 1, 5])
        R.merge_timestep_h(1, 6, 1, 1, 1)                   # no empty slot: the one behind the last written, past the
        assert R.timesteps() == (0, [0, 1, 6])              # current step's and the source's
        same(R.download_timestep(6)[0], wb[0], "capacity 3")
        R.merge_timestep_h(0, 6, 1, 1, 1)                   # a cached output is overwritten in place
        assert R.timesteps() == (0, [0, 1, 6])
        same(R.download_timestep(6)[0], wa[0], "in place")
        R.select_timestep(6)
        R.merge_timestep_h(1, 6, 1, 1, 1)                   # ... the current step too
        assert R.timesteps() == (6, [0, 1, 6])
        same(R.download_timestep()[0], wb[0], "the current step overwritten")
        same(R.download_timestep()[1], wb[1], "the current step overwritten: normals")
        ptrs, keep = field_ptrs(Fa)
        R.upload_timestep_fields_h_device(6, ptrs, 0, dims, 1, 1, 1)   # ... and by the fields form
        assert R.timesteps() == (6, [0, 1, 6])
        same(R.download_timestep()[0], wa[0], "the current step overwritten by the fields form")
        same(R.download_timestep()[1], wa[1], "the current step overwritten by the fields form: normals")
    finally:
        R.close()


def test_merge_on_a_side_stream_behind_a_blend_and_a_source_overwritten(gpu_renderer_factory):
    import torch
    dims = M.SMALL
    for ring, nf in (("u8", 2), ("f32", 2)):
        Fa, Fb, Fc = (H.fields(ring, nf, dims, s) for s in (0, 1, 2))
        a, b, c = H.source_step(Fa, 1), H.source_step(Fb, 1, 6), H.source_step(Fc, 1, 7)
        side, up = torch.cuda.Stream(), torch.cuda.Stream()
        pc, kc = dev(c[0])
        pg, kg = dev(c[1])
        work = out_buffer(1 << 22, np.float32)
        R = context(gpu_renderer_factory, a[0], a[1], cap=5, dm=mode(a[0], 1))
        try:
            R.upload_timestep(1, b[0], b[1], dmode="V2GH")
            torch.cuda.synchronize()                        # nothing is in flight when the two streams start
            with torch.cuda.stream(side):                   # work in front of the blend: nothing behind it has started yet
                for _ in range(24):
                    work.add_(1)
            R.blend_timesteps(0, 1, W, 2, stream=stream_arg(side))
            R.merge_timestep_h(2, 3, 1, 1, 1, stream=stream_arg(side))   # directly behind the blend, no host wait
            R.upload_timestep_device(2, pc, dims, nf + 2, H.CODE[ring], pg, dmode="V2GH",
                                     stream=stream_arg(up))  # the source slot overwritten: behind the merge's reads
            torch.cuda.synchronize()                        # both streams have ended: the host forms below read their results
            got = R.download_timestep(3)
            same(R.download_timestep(2)[0], M.downloaded(*c)[0], "the new step 2")
            R.blend_timesteps(0, 1, W, 2)                   # the synchronous results: the blend again, and the recipe of its fields
            mixed = R.download_timestep(2)
            same(mixed[0], M.downloaded(*T.blend(a[0], a[1], b[0], b[1], np.float32(W)))[0], "the blend")
            Fm = np.ascontiguousarray(mixed[0][..., :nf])
            want = upload_recipe(R, 4, Fm, 1, 1, 1)
        finally:
            R.close()
        same(got[0], want[0], ring + ": data")
        same(got[1], want[1], ring + ": normals")
        ref = H.downloaded(*H.merge_h(Fm, 1, 1, 1))
        same(got[0], ref[0], ring + ": data against the restatement")
        assert not np.array_equal(got[0][..., nf + 1], mixed[0][..., nf + 1]), "vacuous: the blend of H is H of the blend"


def test_refusals(gpu_renderer_factory, smk):
    dims = M.SMALL
    nx, ny, nz = dims
    F = H.fields("u8", 2, dims)
    a = H.source_step(F, 1)
    b = H.source_step(H.fields("u8", 2, dims, 1), 1, 6)
    buf = out_buffer(nx * ny * nz * 4 + 64, np.uint8)
    p0, p1 = buf.data_ptr(), buf.data_ptr() + nx * ny * nz
    mt, up = "smk_merge_timestep_h: ", "smk_upload_timestep_fields_h_device: "
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match=mt + "no volume"):
            R.merge_timestep_h(0, 1)
        with pytest.raises(smk.SmkError, match=up + "no volume"):
            R.upload_timestep_fields_h_device(1, [p0, p1], 0, dims)
        with pytest.raises(smk.SmkError, match="smk_merge_fields_h_device: bad arguments"):
            R.merge_fields_h_device(p0, 3, dims, p1, None, 1, 1, 0)          # three fields leave no room for H
        with pytest.raises(smk.SmkError, match="smk_merge_fields_h_device: bad arguments"):
            R.merge_fields_h_device(p0, 2, dims, p1, None, 1, 1, 2)
        with pytest.raises(smk.SmkError, match="smk_merge_fields_h_f32_device: bad arguments"):
            R.merge_fields_h_f32_device(p0 + 2, 1, dims, p1 + 1, None, 1, 1, 0)   # below float alignment
        with pytest.raises(smk.SmkError, match="smk_merge_fields_h_f32_device: bad arguments"):
            R.merge_fields_h_f32_device(p0, 1, (nx, ny, 2), p0, None, 1, 1, 0)
    finally:
        R.close()
    sca = T.scene(*a)
    fsize = tuple(float(f) for f in sca.fsize)
    R = scene_context(gpu_renderer_factory, sca, cap=2)
    try:
        R.upload_timestep(1, b[0], b[1], fsize=fsize, dmode="V2GH")        # (the data mode of a four-channel scene)
        with Undisturbed(R):                                # a refused call changes nothing: frames, flags, steps
            for args, why in (((99, 5), r"99 \(the source\) is not cached"), ((-1, 5), "is not cached"), ((0, -1), ">= 0"),
                              ((1, 1), "in-place"), ((1, 5), "holds 2 steps.*here 3"), ((0, 5, 2), "add_h 2 is neither 0 nor 1"),
                              ((0, 5, -1), "add_h -1 is neither"), ((0, 5, 1, 1, 2), "blur 2 is neither 0 nor 1"),
                              ((0, 5, 0, 1, -1), "blur -1 is neither")):
                with pytest.raises(smk.SmkError, match=mt + ".*" + why):
                    R.merge_timestep_h(*args)
            for args, why in (((5, None, 0, dims), "d_fields is NULL"), ((5, [p0, None], 0, dims), r"d_fields\[1\] is NULL"),
                              ((5, [p0], 0, dims), "1 fields for a series of nelts 4 with add_h 1"),
                              ((5, [p0, p1], 0, dims, 0), "2 fields for a series of nelts 4 with add_h 0: the fields are nelts - 1 - add_h = 3"),
                              ((5, [p0, p1], 1, dims), r"field_dtype 1 is not the ring's type \(0\)"),
                              ((5, [p0, p1], 7, dims), "field_dtype 7"), ((5, [p0, p1], 0, dims, 3), "add_h 3 is neither"),
                              ((5, [p0, p1], 0, dims, 1, 1, 5), "blur 5 is neither"),
                              ((5, [p0, p1], 0, (nx, ny + 1, nz)), "differ from the series'"), ((-3, [p0, p1], 0, dims), ">= 0")):
                with pytest.raises(smk.SmkError, match=up + ".*" + why):
                    R.upload_timestep_fields_h_device(*args)
        assert R.timesteps() == (0, [0, 1])
        R.merge_timestep_h(0, 5)                            # the only slot that is neither the source's nor current: step 1's
        assert R.timesteps() == (0, [0, 5])
        same(R.download_timestep(5)[0], H.downloaded(*H.merge_h(F, 1, 1, 0))[0], "capacity 2")
    finally:
        R.close()
    # alignment of a field below its element: 16-bit and float rings
    for ring, off, size in (("u16", 1, 2), ("f32", 2, 4)):
        st = H.source_step(H.fields(ring, 1, dims), 1)
        R = scene_context(gpu_renderer_factory, T.scene(*st), cap=3)
        try:
            with Undisturbed(R):
                with pytest.raises(smk.SmkError, match=up + r"d_fields\[0\] is not aligned to its %d-byte" % size):
                    R.upload_timestep_fields_h_device(1, [p0 + off], H.CODE[ring], dims)
            assert R.timesteps() == (0, [0])
        finally:
            R.close()
    # too few channels for the fields, G and H; a u16 voxel that is not one field, G and H
    two = np.ascontiguousarray(a[0][..., :2])
    R = scene_context(gpu_renderer_factory, T.scene(two, a[1]), cap=3)
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match=mt + r"the series has nelts 2: with add_h 1 .*G and H \(nelts >= 3\)"):
                R.merge_timestep_h(0, 1)
            with pytest.raises(smk.SmkError, match=up + "the series has nelts 2: with add_h 1"):
                R.upload_timestep_fields_h_device(1, [p0], 0, dims)
        R.merge_timestep_h(0, 1, 0, 1, 1)                   # (without H it is a field and G)
        assert R.timesteps() == (0, [0, 1])
    finally:
        R.close()
    one = np.ascontiguousarray(a[0][..., :1])
    R = scene_context(gpu_renderer_factory, T.scene(one, a[1]), cap=3)
    try:
        with pytest.raises(smk.SmkError, match=mt + r"the series has nelts 1: with add_h 0 .*one field, G \(nelts >= 2\)"):
            R.merge_timestep_h(0, 1, 0)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    st16 = H.source_step(H.fields("u16", 1, dims), 0)
    R = scene_context(gpu_renderer_factory, T.scene(*st16), cap=3)
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match=mt + "add_h on a 16-bit ring of nelts 2.*nelts 3"):
                R.merge_timestep_h(0, 1)
            with pytest.raises(smk.SmkError, match=up + "add_h on a 16-bit ring of nelts 2"):
                R.upload_timestep_fields_h_device(1, [p0], 2, dims)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    R = scene_context(gpu_renderer_factory, sca, cap=3, shard=(0, 2))
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match=mt + "a sharded context.*reaches 2 voxels beyond region \\+ halo.*three extremes"):
                R.merge_timestep_h(0, 1)
            with pytest.raises(smk.SmkError, match=up + "a sharded context.*reaches 2 voxels"):
                R.upload_timestep_fields_h_device(1, [p0, p1], 0, dims)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    # a cache of one step holds the current step and no other: no slot
    R = scene_context(gpu_renderer_factory, sca)
    try:
        with Undisturbed(R):
            with pytest.raises(smk.SmkError, match=up + "time step 5: the cache holds one step, the current one"):
                R.upload_timestep_fields_h_device(5, [p0, p1], 0, dims)
            with pytest.raises(smk.SmkError, match=mt + "the cache holds 1 steps.*here 2"):
                R.merge_timestep_h(0, 5)
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    # a volume thinner than 3 voxels has no interior voxel
    thin = (np.ascontiguousarray(a[0][:2]), np.ascontiguousarray(a[1][:2]))
    R = scene_context(gpu_renderer_factory, T.scene(*thin), cap=3)
    try:
        with Undisturbed(R, visible=False):
            with pytest.raises(smk.SmkError, match=mt + "a 37x13x2 volume has no interior voxel"):
                R.merge_timestep_h(0, 1)
            with pytest.raises(smk.SmkError, match=up + "a 37x13x2 volume has no interior voxel"):
                R.upload_timestep_fields_h_device(1, [p0, p1], 0, (nx, ny, 2))
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    assert not buf.any()


# ---- 7. the host adapter

def test_host_adapter_shows_the_merged_fields_with_h_of_a_blend(tmp_path):
    """tests/host/merge_h_main drives HipVolumeRenderable::setTimeFraction + setTimeFractionDerivatives over a 3-step two-field
    u8 series with H (GDM_V2GH), with and without setBlurNormals: with derivatives on the step a fractional frame shows is the
    restatement's merge of the blended fields; with them off it is the plain blend"""
    exe = os.path.join(ROOT, "tests", "host", "merge_h_main")
    assert os.path.exists(exe), "%s is not built: __graft_entry__.build() builds it" % exe
    dims = M.SMALL
    nx, ny, nz = dims
    steps = [H.merge_h(H.fields("u8", 2, dims, s), 1, 1, 0) for s in (0, 1, 2)]    # what the host prepared with mergeMV -addH
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
    spec = "%s:%d:%d:%d:4:3:%s" % (d / "s", nx, ny, nz, d / "table.rgba")
    seq = "0:0,0:0.37,0:0.37,1:0.37,1:0"
    order = ((0, 0), (0, .37), (0, .37), (1, .37), (1, 0))

    def run(onoff, blur, name):
        p = subprocess.run([exe, spec, "48", "48", "1", onoff, blur, seq, str(d / name)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert "ERROR" not in p.stderr, p.stderr
        n = sum(line.startswith("frame ") for line in p.stdout.splitlines())
        assert n == len(order)
        return [np.fromfile("%s.%d.f32" % (d / name, k), np.float32) for k in range(n)]

    def shown(name, k):
        return (np.fromfile("%s.%d.data" % (d / name, k), np.uint8).reshape(nz, ny, nx, 4),
                np.fromfile("%s.%d.grad" % (d / name, k), np.uint8).reshape(nz, ny, nx, 3))
    frames = {(o, b): run(o, b, o + b) for o, b in (("on", "plain"), ("on", "blur"), ("off", "blur"))}
    assert max(f.max() for f in frames[("on", "plain")]) > 0.05
    for k, (t, f) in enumerate(order):
        mixed = T.blend(steps[t][0], steps[t][1], steps[t + 1][0], steps[t + 1][1], np.float32(f)) if f else steps[t]
        Fm = np.ascontiguousarray(mixed[0][..., :2])
        for (o, b), _ in frames.items():
            want = H.merge_h(Fm, 1, 1, int(b == "blur")) if f and o == "on" else mixed
            got = shown(o + b, k)
            same(got[0], want[0], "%s %s, draw %d: data" % (o, b, k))
            same(got[1], want[1], "%s %s, draw %d: normals" % (o, b, k))
        if f:
            p, q = H.merge_h(Fm, 1, 1, 0), H.merge_h(Fm, 1, 1, 1)
            assert not np.array_equal(p[0], mixed[0]) and not np.array_equal(p[1], q[1]) and np.array_equal(p[0], q[0]), "vacuous"
            assert not np.array_equal(p[0][..., 3], mixed[0][..., 3]), "vacuous: the blend of H is H of the blend"
        else:                                               # (a whole step is the same frame either way)
            assert np.array_equal(frames[("on", "plain")][k], frames[("off", "blur")][k]), "draw %d" % k
    on = frames[("on", "plain")]
    assert np.array_equal(on[1], on[2]) and not np.array_equal(on[1], on[3])


def test_host_adapter_hands_blur_to_the_derive_and_to_the_merge_without_h(tmp_path, O):
    """setBlurNormals on three-channel series: a GDM_V2G series shows the merge of the blended fields with blurred normals
    (smk_merge_timestep_h, add_h 0), a GDM_VGH series the derive of the blended scalar with blurred normals"""
    import _step_derive_ref as V
    exe = os.path.join(ROOT, "tests", "host", "merge_h_main")
    assert os.path.exists(exe), "%s is not built: __graft_entry__.build() builds it" % exe
    dims = M.SMALL
    nx, ny, nz = dims
    series = {"V2G": [H.merge_h(H.fields("u8", 2, dims, s), 0, 1, 0) for s in (0, 1, 2)],
              "VGH": [V.series_step(O, V.scalar(s, dims), "u8") for s in (0, 1, 2)]}
    tex = np.zeros((256, 256, 4), np.uint8)
    tex[..., 0] = np.arange(256, dtype=np.uint8)[None, :]
    tex[..., 2] = 90
    tex[..., 3] = 60
    tex.tofile(str(tmp_path / "table.rgba"))
    order = ((0, 0), (0, .37), (1, .6))
    for mode, steps in series.items():
        for t, (data, nrm) in enumerate(steps):
            data.tofile(str(tmp_path / ("%s.%d.mf" % (mode, t))))
            nrm.tofile(str(tmp_path / ("%s.%d.nrm" % (mode, t))))
        spec = "%s:%d:%d:%d:3:3:%s" % (tmp_path / mode, nx, ny, nz, tmp_path / "table.rgba")
        out = str(tmp_path / ("out" + mode))
        p = subprocess.run([exe, spec, "48", "48", "1", "on", "blur", "0:0,0:0.37,1:0.6", out, mode], capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0 and "ERROR" not in p.stderr, p.stderr
        for k, (t, f) in enumerate(order):
            mixed = T.blend(steps[t][0], steps[t][1], steps[t + 1][0], steps[t + 1][1], np.float32(f)) if f else steps[t]
            if not f:
                want = plain = mixed
            elif mode == "V2G":
                Fm = np.ascontiguousarray(mixed[0][..., :2])
                want, plain = H.merge_h(Fm, 0, 1, 1), H.merge_h(Fm, 0, 1, 0)
            else:
                s = np.ascontiguousarray(mixed[0][..., 0])
                want, plain = V.derive(O, s, "u8", 1, 1), V.derive(O, s, "u8", 1, 0)
            got = (np.fromfile("%s.%d.data" % (out, k), np.uint8).reshape(nz, ny, nx, 3),
                   np.fromfile("%s.%d.grad" % (out, k), np.uint8).reshape(nz, ny, nx, 3))
            same(got[0], want[0], "%s, draw %d: data" % (mode, k))
            same(got[1], want[1], "%s, draw %d: normals" % (mode, k))
            if f:
                assert not np.array_equal(want[1], plain[1]) and np.array_equal(want[0], plain[0]), "vacuous"
