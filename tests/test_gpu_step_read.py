"""A resident time step read back (smk.h smk_get_timestep_box / smk_download_timestep_device / smk_download_timestep): every
stored field of every voxel, exactly, against the NumPy restatement of the header's contract (tests/_step_read_ref.py,
qualified by tests/test_step_read_cpu.py) -- every packed layout with and without normals, bricked uploads, every shard,
steps that are not current, uploaded from device memory on another stream, overwritten behind the read, blended in time --
and the two things the entry exists for: a step that goes into a fresh context and renders the same frame, and the
derivatives of a blended scalar made on the device.  Volumes are per-voxel noise; f32 voxels are compared as their 32-bit
patterns.  Every output buffer of a _device call lies between 64 guard bytes of 0xA5 that must not change."""
import numpy as np
import pytest

import _step_hist_ref as S
import _step_read_ref as D
import _tblend_ref as T
from _gpu_mem import Guarded, busy, dev_tensor as dev, out_buffer, stream_arg
from _layouts import shuffled
from _step_gpu import bricked, context, ring, same_bits as same

pytestmark = pytest.mark.gpu
BIG = S.DIMS                                                # 41 x 37 x 45


def guarded_buffers(R, want_grad=True, shift=0):
    """the guarded buffers a download of a step of R's series takes: (data's, normals' or None, a function that reads them).
    Making them waits for the device (Guarded), so a test that lets no host wait between two calls makes them first"""
    _, (sx, sy, sz), ne, dt, _ = R.timestep_box()
    nv = sx * sy * sz
    gd = Guarded(nv * ne * dt.itemsize, shift * dt.itemsize)
    gg = Guarded(nv * 3, shift) if want_grad else None

    def read():
        return gd.take(dt, (sz, sy, sx, ne), "data"), (gg.take(np.uint8, (sz, sy, sx, 3), "grad") if gg else None)
    return gd, gg, read


def download_device(R, step=-1, stream=None, want_grad=True, shift=0, sync=True, bufs=None):
    """download_timestep_device into guarded buffers (bufs, or new ones) -> (data, grad or None); sync False: (the buffers, a
    function that reads them), and with bufs given the call enqueues the download and waits for nothing"""
    import torch
    gd, gg, read = bufs or guarded_buffers(R, want_grad, shift)
    R.download_timestep_device(gd.ptr, gg.ptr if gg else None, step, stream)
    if not sync:
        return (gd, gg), read
    torch.cuda.synchronize()                                # the download ran on the context's stream, or the caller's: read-back
    return read()


def both_forms(R, want, wgrad, what, step=-1, shift=0):
    data, grad = R.download_timestep(step)
    same(data, want, what + ": host form, data")
    same(grad, wgrad, what + ": host form, normals")
    data, grad = download_device(R, step, shift=shift)
    same(data, want, what + ": device form, data")
    same(grad, wgrad, what + ": device form, normals")


# ---- 1. layouts

@pytest.mark.parametrize("normals", [True, False], ids=["normals", "no-normals"])
@pytest.mark.parametrize("dtype, nelts", D.LAYOUTS)
def test_layouts(gpu_renderer_factory, dtype, nelts, normals):
    data, grad = D.volume(dtype, nelts)
    grad = grad if normals else None
    want, wgrad = D.expected(data, grad)
    assert normals or (wgrad == 128).all()
    R = context(gpu_renderer_factory, data, grad)
    try:
        assert R.timestep_box() == ((0, 0, 0), D.SMALL, nelts, np.dtype(D.NP[dtype]), normals)
        both_forms(R, want, wgrad, "%s x %d" % (dtype, nelts))
        # the output moved to the other phases of its 16-byte line
        for shift in (1, 2, 3, 5):
            d2, g2 = download_device(R, shift=shift)
            same(d2, want, "shift %d: data" % shift)
            same(g2, wgrad, "shift %d: normals" % shift)
        # the voxels alone
        d3, g3 = download_device(R, want_grad=False)
        assert g3 is None
        same(d3, want, "without normals asked for")
        same(R.download_timestep(want_grad=False)[0], want, "host form without normals asked for")
    finally:
        R.close()


@pytest.mark.parametrize("dtype, dims", [("u8", D.LONG), ("f32", D.LONG), ("u8", D.LONGER), ("u16", D.LONGER)])
def test_rows_longer_than_a_workgroups_run(gpu_renderer_factory, dtype, dims):
    data, grad = D.volume(dtype, 3, dims)
    R = context(gpu_renderer_factory, data, grad)
    try:
        both_forms(R, *D.expected(data, grad), what="%s %s" % (dtype, dims), shift=1)
    finally:
        R.close()


# ---- 2. bricked and shuffled uploads

@pytest.mark.parametrize("dtype, nelts", [("u8", 3), ("f32", 4), ("u16", 3)])
def test_bricked_and_shuffled_upload(gpu_renderer_factory, smk, dtype, nelts):
    data, grad = D.volume(dtype, nelts, BIG)
    want, wgrad = D.expected(data, grad)
    for order in (list(range(8)), shuffled(8)):
        R = gpu_renderer_factory()
        try:
            descs, keep = bricked(smk, data, grad, order)
            R._ck(R.L.smk_upload_volume(R.ctx, descs, len(descs), nelts, D.CODE[dtype], smk.binding.GDM[D.DMODE[nelts]]))
            both_forms(R, want, wgrad, "bricks in order %s" % order)
        finally:
            R.close()


# ---- 3. shards

@pytest.mark.parametrize("dtype, nelts", [("u8", 3), ("f32", 4), ("u16", 3)])
@pytest.mark.parametrize("nranks", [2, 4, 8])
def test_shards(gpu_renderer_factory, dtype, nelts, nranks):
    data, grad = D.volume(dtype, nelts, BIG)
    want, wgrad = D.expected(data, grad)
    whole = {h: (np.zeros_like(want), np.zeros_like(wgrad)) for h in (1, 3)}
    written = {h: np.zeros(want.shape[:3], np.int32) for h in (1, 3)}
    for halo in (1, 3):
        for rank in range(nranks):
            g0, g1 = D.region(BIG, rank, nranks)
            size = tuple(g1[a] - g0[a] for a in range(3))
            R = context(gpu_renderer_factory, data, grad, shard=(rank, nranks), halo=halo)
            try:
                assert R.timestep_box() == (g0, size, nelts, np.dtype(D.NP[dtype]), True), (rank, nranks, halo)
                what = "rank %d of %d, halo %d" % (rank, nranks, halo)
                both_forms(R, D.cut(want, g0, g1), D.cut(wgrad, g0, g1), what)
                d, g = R.download_timestep()
            finally:
                R.close()
            box = (slice(g0[2], g1[2]), slice(g0[1], g1[1]), slice(g0[0], g1[0]))
            whole[halo][0][box], whole[halo][1][box] = d, g
            written[halo][box] += 1
        assert (written[halo] == 1).all()
        same(whole[halo][0], want, "the ranks' boxes at their origins, halo %d" % halo)
        same(whole[halo][1], wgrad, "... their normals")
    same(whole[1][0], whole[3][0], "the halo size changes nothing returned")


# ---- 4. the ring

@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
def test_steps_by_id_and_current(gpu_renderer_factory, dtype):
    R, a, b = ring(gpu_renderer_factory, D.volume(dtype, 3, D.SMALL, 1), D.volume(dtype, 3, D.SMALL, 2))
    ea, eb = D.expected(*a), D.expected(*b)
    assert not np.array_equal(D.bits(ea[0]), D.bits(eb[0]))
    try:
        both_forms(R, *eb, what="a cached step that is not current", step=1)
        both_forms(R, *ea, what="the current step by id", step=0)
        both_forms(R, *ea, what="SMK_STEP_CURRENT")
        R.select_timestep(1)
        both_forms(R, *eb, what="SMK_STEP_CURRENT after a switch")
        both_forms(R, *ea, what="the step left behind", step=0)
    finally:
        R.close()


def test_device_upload_on_one_stream_download_on_another(gpu_renderer_factory):
    import torch
    a, b = D.volume("u8", 3, BIG, 1), D.volume("u8", 3, BIG, 2)
    up, ds = torch.cuda.Stream(), torch.cuda.Stream()
    work = out_buffer(1 << 28, np.uint8)
    d, g = dev(b[0]), dev(b[1])
    R = context(gpu_renderer_factory, a[0], a[1], cap=2)
    try:
        bufs = guarded_buffers(R)                           # (made before the streams start: making them waits for the device)
        torch.cuda.synchronize()                            # nothing is in flight when the two streams start
        busy(up, work)
        R.upload_timestep_device(5, d.data_ptr(), BIG, 3, 0, g.data_ptr(), dmode="VGH", stream=stream_arg(up))
        _, read = download_device(R, 5, stream_arg(ds), sync=False, bufs=bufs)     # no host wait in between
        ds.synchronize()                                    # the download's stream alone: it waited for the upload on the device
        data, grad = read()
        same(data, b[0], "the step uploaded on the other stream")
        same(grad, b[1], "... its normals")
        torch.cuda.synchronize()                            # stream `up` has ended before its work buffer goes
    finally:
        R.close()


def test_an_upload_into_the_slot_waits_for_the_download(gpu_renderer_factory):
    import torch
    a, b, c = (D.volume("f32", 2, BIG, s) for s in (1, 2, 3))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    work = out_buffer(1 << 28, np.uint8)
    d, g = dev(c[0]), dev(c[1])
    R = context(gpu_renderer_factory, a[0], a[1], cap=2)
    try:
        R.upload_timestep(5, b[0], b[1], dmode="V1G")
        bufs = guarded_buffers(R)                           # (made before the streams start: making them waits for the device)
        torch.cuda.synchronize()                            # nothing is in flight when the two streams start
        busy(s1, work)
        _, read = download_device(R, 5, stream_arg(s1), sync=False, bufs=bufs)     # behind the busy work, no host wait
        R.upload_timestep_device(5, d.data_ptr(), BIG, 2, 1, g.data_ptr(), dmode="V1G", stream=stream_arg(s2))
        torch.cuda.synchronize()                            # both streams: read-back
        data, grad = read()
        same(data, b[0], "the step the download was asked of")
        same(grad, b[1], "... its normals")
        both_forms(R, *D.expected(*c), what="the step that replaced it", step=5)
    finally:
        R.close()


# ---- 5. a blended step, field by field

@pytest.mark.parametrize("w", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("dtype, nelts", [("u8", 4), ("u16", 3), ("f32", 3), ("f32", 4)])
def test_blended_step_field_by_field(gpu_renderer_factory, dtype, nelts, w):
    dims = (21, 13, 7)
    a, b = (D.volume(dtype, nelts, dims, s, False) for s in (1, 2))     # (finite floats: the blend is arithmetic)
    R = context(gpu_renderer_factory, a[0], a[1], cap=4)
    try:
        R.upload_timestep(1, b[0], b[1], dmode=D.DMODE[nelts])
        R.blend_timesteps(0, 1, w, 7)
        want, wgrad = T.blend(a[0], a[1], b[0], b[1], w)                # (a u16 third channel: 257 x the blended 8-bit field)
        if w in (0.0, 1.0):
            end = D.expected(*(a if w == 0.0 else b))
            same(want, end[0], "the restatement at w = %g" % w)
            same(wgrad, end[1], "the restatement's normals at w = %g" % w)
        else:
            assert not np.array_equal(D.bits(want), D.bits(D.expected(*a)[0]))
        both_forms(R, want, wgrad, "blend at w = %g" % w, step=7)
    finally:
        R.close()


# ---- 6. closure: what comes back goes up again as the same step

@pytest.mark.parametrize("dtype, nelts", [("u8", 3), ("u16", 3), ("f32", 4)])
def test_a_downloaded_step_uploads_as_the_same_step(gpu_renderer_factory, dtype, nelts):
    import _layouts as L
    dims = L.DIMS_ODD
    data, grad = D.volume(dtype, nelts, dims, 1, False)
    sc = L.scene(3, False, "2d", shade=1, view="rot", window=(48, 48), steps=48, dims=dims)     # the frame's state alone

    def shoot(R):
        L.frame_state(R, sc)
        R.set_option("kernel", 1)                           # the gather kernel
        return R.render(), R.hist2d_step()

    R = context(gpu_renderer_factory, data, grad)
    try:
        d1, g1 = R.download_timestep()
        frame1, hist1 = shoot(R)
    finally:
        R.close()
    assert frame1[..., 3].max() > 0.05, "vacuous: an empty frame"
    if dtype == "u16":
        assert not np.array_equal(d1[..., 2], data[..., 2])
    R = context(gpu_renderer_factory, d1, g1)
    try:
        d2, g2 = R.download_timestep()
        frame2, hist2 = shoot(R)
    finally:
        R.close()
    same(d2, d1, "the voxels, downloaded again")
    same(g2, g1, "the normals, downloaded again")
    same(hist2, hist1, "the step histogram")
    same(frame2, frame1, "the frame")


# ---- 7. the promised recipe: derivatives of a blend, on the device

def test_derivatives_of_a_blend_on_the_device(gpu_renderer_factory, O):
    import torch
    dims = (24, 20, 18)
    nx, ny, nz = dims
    w = 0.37
    rng = np.random.default_rng(24)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    scal = [np.clip(np.sin(x * (.3 + .1 * s)) * 60 + np.cos(y * .2 + z * .5 + s) * 50 + 128 + rng.normal(0, 4, x.shape), 0, 255)
            .astype(np.uint8) for s in (0, 1)]
    steps = []
    for v in scal:                                          # the series the host prepared: VGH and normals of each scalar
        vgh = O.make_vgh(v)
        steps.append((vgh, O.normals_vgh(vgh, blur=False)))
    mixed = T.blend(steps[0][0], steps[0][1], steps[1][0], steps[1][1], w)[0][..., 0]      # the blended SCALAR
    want_vgh = O.make_vgh(np.ascontiguousarray(mixed))
    want_nrm = O.normals_vgh(want_vgh, blur=False)
    assert not np.array_equal(want_vgh[..., 1:], T.blend(steps[0][0], None, steps[1][0], None, w)[0][..., 1:]), \
        "vacuous: the blend of G and H is G and H of the blend"
    R = context(gpu_renderer_factory, steps[0][0], steps[0][1], cap=4)
    try:
        R.upload_timestep(1, steps[1][0], steps[1][1], dmode="VGH")
        R.blend_timesteps(0, 1, w, 2)
        nv = nx * ny * nz
        gd = Guarded(nv * 3)
        R.download_timestep_device(gd.ptr, None, 2)         # (on the context's stream, as the prep entries below)
        torch.cuda.synchronize()                            # torch's stream is not the context's: wait on both sides of its copy
        s0 = gd.t[gd.off:gd.off + nv * 3].view(nz, ny, nx, 3)[..., 0].contiguous()         # channel 0, a strided device copy
        vgh = out_buffer((nz, ny, nx, 3), np.uint8)
        nrm = out_buffer((nz, ny, nx, 3), np.uint8)           # (these wait for s0's copy too)
        R.make_vgh_device(s0.data_ptr(), 0, dims, 1, vgh.data_ptr(), None)
        R.normals_vgh_device(vgh.data_ptr(), 3, dims, 0, nrm.data_ptr())
        R.upload_timestep_device(3, vgh.data_ptr(), dims, 3, 0, nrm.data_ptr(), dmode="VGH")
        got, gnrm = R.download_timestep(3)
        gd.take(np.uint8, (nv * 3,), "the blend's download")
    finally:
        R.close()
    same(got, want_vgh, "VGH of the blended scalar")
    same(gnrm, want_nrm, "its normals")


# ---- 8. refusals

def test_refusals(gpu_renderer_factory, smk):
    buf = out_buffer(1 << 16, np.uint8)
    R = gpu_renderer_factory()
    try:
        host = np.zeros(16, np.uint8)
        with pytest.raises(smk.SmkError, match="smk_download_timestep: no volume"):
            R._ck(R.L.smk_download_timestep(R.ctx, -1, host.ctypes.data, None))
        with pytest.raises(smk.SmkError, match="smk_download_timestep_device: no volume"):
            R.download_timestep_device(buf.data_ptr())
        with pytest.raises(smk.SmkError, match="smk_get_timestep_box: no volume"):
            R.timestep_box()
    finally:
        R.close()
    data, grad = D.volume("f32", 2)
    R = context(gpu_renderer_factory, data, grad)
    try:
        for step in (7, -2):
            with pytest.raises(smk.SmkError, match="time step %d is not cached" % step):
                R.download_timestep(step)
            with pytest.raises(smk.SmkError, match="time step %d is not cached" % step):
                R.download_timestep_device(buf.data_ptr(), None, step)
        with pytest.raises(smk.SmkError, match="d_data is NULL"):
            R.download_timestep_device(None)
        assert R.L.smk_download_timestep(R.ctx, -1, None, None) != 0
        assert b"data is NULL" in R.L.smk_last_error(R.ctx)
        with pytest.raises(smk.SmkError, match="not aligned"):
            R.download_timestep_device(buf.data_ptr() + 2)
        assert not buf.any()                                # nothing was written by a refused call
        both_forms(R, *D.expected(data, grad), what="after the refusals")
    finally:
        R.close()
