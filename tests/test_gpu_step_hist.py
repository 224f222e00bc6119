"""The joint histogram of a RESIDENT time step (smk.h smk_hist2d_step_device / smk_hist2d_step), read from the context's packed
voxels: raw COUNTS, exactly, against the NumPy restatement of the header's contract (tests/_step_hist_ref.py, qualified by
tests/test_step_hist_cpu.py) -- for every packed layout, bricked uploads, every shard, steps that are not current, uploaded
from device memory on another stream or blended in time -- and, where the older entries apply (u8, f32), their bytes.  The
volume is 41 x 37 x 45 (tests/_step_hist_ref.DIMS): all odd, more than one flush chunk."""
import numpy as np
import pytest

import _step_hist_ref as S
import _tblend_ref as T
from _gpu_mem import busy, dev_tensor as dev, out_buffer, stream_arg
from _layouts import shuffled
from _step_gpu import bricked, context, ring, same_bins as same

pytestmark = pytest.mark.gpu
DMODE = {1: "V1", 2: "V1G", 3: "VGH", 4: "V2GH"}
DT = {"u8": 0, "f32": 1, "u16": 2}
NX, NY, NZ = S.DIMS
NVOX = NX * NY * NZ
LAYOUTS = [("u8", 2), ("u8", 3), ("u8", 4), ("f32", 2), ("f32", 3), ("f32", 4), ("u16", 2), ("u16", 3)]


# ---- 1. layouts

@pytest.mark.parametrize("dtype, nelts", LAYOUTS)
def test_layouts(gpu_renderer_factory, smk, dtype, nelts):
    data, grad = S.volume(dtype, nelts)
    want = S.counts(data)
    assert int(want.sum()) == NVOX > S.CHUNK
    R = context(gpu_renderer_factory, data, grad)
    try:
        got, hist = R.hist2d_step(want="both")
        same(got, want, "counts")
        same(hist, S.finish(want), "bytes")
        same(R.hist2d_step(want="hist"), hist, "bytes alone")
        if dtype == "u8":                                   # the entry for the host's raw array is the yardstick
            same(hist, R.hist2d(data), "smk_hist2d")
        if dtype == "f32":
            d = dev(data)
            same(hist, R.hist2d_f32_device(d.data_ptr(), nelts, S.DIMS), "smk_hist2d_f32_device")
    finally:
        R.close()
    # the same volume handed over as 2 x 2 x 2 bricks in another order
    R = gpu_renderer_factory()
    try:
        descs, keep = bricked(smk, data, grad, shuffled(8))
        R._ck(R.L.smk_upload_volume(R.ctx, descs, len(descs), nelts, DT[dtype], smk.binding.GDM[DMODE[nelts]]))
        same(R.hist2d_step(), want, "bricked")
    finally:
        R.close()


def test_no_normals_and_an_even_volume(gpu_renderer_factory):
    for dtype in ("u8", "f32", "u16"):
        data = np.ascontiguousarray(S.volume(dtype, 2)[0][:44, :36, :40])
        R = context(gpu_renderer_factory, data, None)
        try:
            same(R.hist2d_step(), S.counts(data), dtype)
        finally:
            R.close()


def test_more_chunks_than_workgroups(gpu_renderer_factory):
    """the kernel runs at most 256 workgroups, which stride over the flush chunks: 16.4 M voxels are 268 chunks, so some
    workgroups take a second one (the smallest size at which that loop turns twice)"""
    nx, ny, nz = 255, 251, 257
    assert nx * ny * nz > 256 * S.CHUNK
    rng = np.random.default_rng(77)
    data = rng.integers(0, 256, (nz, ny, nx, 2), dtype=np.uint8)
    data[:, :, :, 1] >>= 2                                  # (64 x 256 bins: counts of a few thousand each)
    data[:40] = (1, 2)
    want = S.counts(data)
    R = context(gpu_renderer_factory, data, None)
    try:
        got, hist = R.hist2d_step(want="both")
        same(got, want, "counts")
        same(hist, R.hist2d(data), "smk_hist2d")
    finally:
        R.close()


# ---- 2. the wave-uniform path

@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
def test_a_constant_volume_with_one_other_voxel(gpu_renderer_factory, dtype):
    data = np.zeros((NZ, NY, NX, 2), S.volume(dtype, 2)[0].dtype)
    data[...] = {"u8": (9, 200), "f32": (0.25, 0.75), "u16": (9 * 257, 200 * 257 + 100)}[dtype]
    data[NZ // 2, NY // 2, NX // 2] = {"u8": (10, 200), "f32": (0.5, 0.75), "u16": (10 * 257, 200 * 257)}[dtype]
    R = context(gpu_renderer_factory, data, None)
    try:
        got = R.hist2d_step()
    finally:
        R.close()
    same(got, S.counts(data))
    assert np.count_nonzero(got) == 2 and sorted(got[got > 0]) == [1, NVOX - 1]


# ---- 3. f32 specials, 4. u16 edges

def test_f32_specials(gpu_renderer_factory):
    data = S.volume("f32", 2)[0].copy()
    flat = data.reshape(-1, 2)
    plants = np.array([np.nan, np.inf, -np.inf, -0.25, -0.0, 1.0, 1.5, 254.999 / 255, 3.0e38, -3.0e38], np.float32)
    n = len(plants)
    at = 20000                                              # (past the uniform slices)
    flat[at:at + n, 0] = plants
    flat[at + n:at + 2 * n, 1] = plants
    flat[at + 2 * n:at + 3 * n] = plants[:, None]
    want = S.counts(data)
    assert list(S.bin_f32(plants)) == [0, 255, 0, 0, 0, 255, 255, 254, 255, 0]     # (the rule: +inf * 255 >= 255)
    R = context(gpu_renderer_factory, data, None)
    try:
        same(R.hist2d_step(), want)
    finally:
        R.close()


def test_u16_edges(gpu_renderer_factory):
    data = np.zeros((NZ, NY, NX, 2), np.uint16)
    data[...] = (40 * 257, 50 * 257)
    flat = data.reshape(-1, 2)
    for i, (v, _) in enumerate(S.U16_EDGES):
        flat[1000 + 97 * i] = (v, 50 * 257)
        flat[30001 + 97 * i] = (40 * 257, v)
    R = context(gpu_renderer_factory, data, None)
    try:
        got = R.hist2d_step()
    finally:
        R.close()
    same(got, S.counts(data))
    for v, b in S.U16_EDGES:
        assert got[50, b] == (2 if b in (0, 1) else 1) and got[b, 40] == (2 if b in (0, 1) else 1), (v, b)


# ---- 5. shards

@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("nranks, halo", S.SHARD_CASES)
def test_shards(gpu_renderer_factory, smk, dtype, nranks, halo):
    from simian_spacemonkey_amd import sortlast
    data, grad = S.volume(dtype, 3)
    whole = S.counts(data)
    total = np.zeros((256, 256), np.int64)
    for rank in range(nranks):
        R = context(gpu_renderer_factory, data, grad, shard=(rank, nranks), halo=halo)
        try:
            got = R.hist2d_step()
        finally:
            R.close()
        same(got, S.counts(data, *sortlast.shard_region(S.DIMS, rank, nranks)), "rank %d of %d, halo %d" % (rank, nranks, halo))
        total += got
    same(total, whole, "sum over the ranks")
    same(smk.Renderer.hist2d_finish(total), S.finish(whole), "finished sum")


# ---- 6. steps

@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
def test_steps_by_id_current_and_blended(gpu_renderer_factory, dtype):
    R, a, b = ring(gpu_renderer_factory, S.volume(dtype, 3, 1), S.volume(dtype, 3, 2))
    ca, cb = S.counts(a[0]), S.counts(b[0])
    assert not np.array_equal(ca, cb)
    try:
        same(R.hist2d_step(1), cb, "a cached step that is not current")
        same(R.hist2d_step(0), ca, "the current step by id")
        same(R.hist2d_step(), ca, "SMK_STEP_CURRENT")
        R.select_timestep(1)
        same(R.hist2d_step(), cb, "SMK_STEP_CURRENT after a switch")
        same(R.hist2d_step(0), ca, "the step left behind")
        R.blend_timesteps(0, 1, 0.3, 10)
        mid = T.blend(a[0], a[1], b[0], b[1], 0.3)[0]
        cm = S.counts(mid)
        assert not np.array_equal(cm, ca) and not np.array_equal(cm, cb)
        same(R.hist2d_step(10), cm, "a blended step")
        same(R.hist2d_step(), cb, "... which did not become current")
        R.select_timestep(10)
        same(R.hist2d_step(), cm, "the blended step, current")
    finally:
        R.close()


def test_device_upload_on_one_stream_histogram_on_another(gpu_renderer_factory):
    import torch
    a, b = S.volume("u8", 3, 1), S.volume("u8", 3, 2)
    up, hs = torch.cuda.Stream(), torch.cuda.Stream()
    work = out_buffer(1 << 28, np.uint8)
    d, g = dev(b[0]), dev(b[1])
    cnt = out_buffer(65536, np.int32, -1)
    R = context(gpu_renderer_factory, a[0], a[1], cap=2)
    try:
        torch.cuda.synchronize()                            # nothing is in flight when the two streams start
        busy(up, work)
        R.upload_timestep_device(5, d.data_ptr(), S.DIMS, 3, 0, g.data_ptr(), dmode="VGH", stream=stream_arg(up))
        R.hist2d_step_device(cnt.data_ptr(), 5, stream_arg(hs))        # no host wait in between
        hs.synchronize()                                    # the histogram's stream alone: it waited for the upload on the device
        same(cnt.cpu().numpy().view(np.uint32).reshape(256, 256), S.counts(b[0]))
        torch.cuda.synchronize()                            # stream `up` has ended before its work buffer goes
    finally:
        R.close()


def test_an_upload_into_the_slot_waits_for_the_histogram(gpu_renderer_factory):
    import torch
    a, b, c = (S.volume("f32", 2, s) for s in (1, 2, 3))
    hs, up = torch.cuda.Stream(), torch.cuda.Stream()
    work = out_buffer(1 << 28, np.uint8)
    d, g = dev(c[0]), dev(c[1])
    cnt = out_buffer(65536, np.int32, -1)
    R = context(gpu_renderer_factory, a[0], a[1], cap=2)
    try:
        R.upload_timestep(5, b[0], b[1], dmode="V1G")
        torch.cuda.synchronize()                            # nothing is in flight when the two streams start
        busy(hs, work)
        R.hist2d_step_device(cnt.data_ptr(), 5, stream_arg(hs))
        R.upload_timestep_device(5, d.data_ptr(), S.DIMS, 2, 1, g.data_ptr(), dmode="V1G", stream=stream_arg(up))
        torch.cuda.synchronize()                            # both streams: read-back
        same(cnt.cpu().numpy().view(np.uint32).reshape(256, 256), S.counts(b[0]), "the step the histogram was asked of")
        same(R.hist2d_step(5), S.counts(c[0]), "the step that replaced it")
    finally:
        R.close()


# ---- 7. the device form

def test_device_counts_are_overwritten(gpu_renderer_factory):
    import torch
    data, grad = S.volume("u16", 2)
    want = S.counts(data)
    cnt = out_buffer(65536, np.int32, 0x5a5a5a5a)
    R = context(gpu_renderer_factory, data, grad)
    try:
        for turn in range(2):
            R.hist2d_step_device(cnt.data_ptr())
            torch.cuda.synchronize()                        # the context's stream: read-back
            same(cnt.cpu().numpy().view(np.uint32).reshape(256, 256), want, "call %d" % turn)
    finally:
        R.close()


# ---- 8. refusals

def test_refusals(gpu_renderer_factory, smk):
    cnt = out_buffer(65536, np.int32)
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match="smk_hist2d_step: no volume"):
            R.hist2d_step()
        with pytest.raises(smk.SmkError, match="smk_hist2d_step_device: no volume"):
            R.hist2d_step_device(cnt.data_ptr())
    finally:
        R.close()
    data, grad = S.volume("u8", 2)
    R = context(gpu_renderer_factory, np.ascontiguousarray(data[..., :1]), grad)
    try:
        with pytest.raises(smk.SmkError, match="needs value and gradient channels"):
            R.hist2d_step()
    finally:
        R.close()
    R = context(gpu_renderer_factory, data, grad)
    try:
        for step in (7, -2):
            with pytest.raises(smk.SmkError, match="time step %d is not cached" % step):
                R.hist2d_step(step)
            with pytest.raises(smk.SmkError, match="time step %d is not cached" % step):
                R.hist2d_step_device(cnt.data_ptr(), step)
        with pytest.raises(smk.SmkError, match="d_counts is NULL"):
            R.hist2d_step_device(None)
        assert R.L.smk_hist2d_step(R.ctx, -1, None, None) != 0
        assert b"neither counts nor hist" in R.L.smk_last_error(R.ctx)
        with pytest.raises(ValueError):
            R.hist2d_step(want="bytes")
        same(R.hist2d_step(), S.counts(data), "after the refusals")
    finally:
        R.close()
