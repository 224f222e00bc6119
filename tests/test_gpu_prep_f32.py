"""The float data-preparation entries (smk_normals_f32_device, smk_merge_fields_f32_device, smk_hist2d_f32_device)
against tests/_prep_f32_ref.py, the NumPy float32 restatement that tests/test_prep_f32_ref.py ties to the checker:
the contracts are plain fp32, so the bar is np.array_equal."""
import functools

import numpy as np
import pytest

import _prep_f32_ref as P
from _scenes import make_scene, push_scene, tf_cfg3

pytestmark = pytest.mark.gpu

# one interior voxel; ragged; more voxels than the 256 * 32 * 256 threads of one grid pass (a second grid-stride turn)
SHAPES = [(3, 3, 3), (40, 24, 18), (129, 128, 128)]
assert 129 * 128 * 128 > 256 * 32 * 256


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def _dev(t):
    import torch
    return torch.from_numpy(np.array(t, order="C")).cuda()          # (a copy: the shared references are read-only)


def _zeros(shape, dtype):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype), device="cuda")


@functools.lru_cache(maxsize=None)
def smooth_field(dims, seed=0, plant=True):
    """[z][y][x] f32: analytic shells plus rng.random * 0.2 (no multiples of 1/255); with `plant`, where there is room,
    one NaN and one +inf voxel inside and a flat patch (zero gradient)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(100 + seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r = np.sqrt(((x + .5) / nx - .5) ** 2 + ((y + .5) / ny - .47) ** 2 + ((z + .5) / nz - .52) ** 2)
    v = (0.4 + 0.35 * np.cos((9 + seed) * r) + rng.random(r.shape) * 0.2).astype(np.float32)
    if plant and min(dims) >= 12:
        v[nz // 2, ny // 2, nx // 2] = np.nan
        v[nz // 3, ny // 3, nx // 3] = np.inf
        v[2:7, 3:8, 2:8] = 0.3125
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def normals_case(dims, blur):
    """(channel 0, the restatement's normals): shared by the nelts 1 and 3 cases, which differ in the stride alone"""
    v = smooth_field(dims)
    ref = P.normals_f32(v[..., None], blur=bool(blur))
    if min(dims) >= 12:
        assert len(np.unique(ref[:18].reshape(-1, 3), axis=0)) > 1000
    ref.setflags(write=False)
    return v, ref


@pytest.mark.parametrize("nelts", [1, 3])
@pytest.mark.parametrize("blur", [0, 1])
@pytest.mark.parametrize("dims", SHAPES)
def test_normals_f32_bit_exact(R, dims, blur, nelts):
    nx, ny, nz = dims
    v, ref = normals_case(dims, blur)
    vol = np.empty((nz, ny, nx, nelts), np.float32)
    vol[...] = np.float32(-7.25)            # (channels the entry must not read)
    vol[..., 0] = v
    out = _zeros((nz, ny, nx, 3), "uint8")
    R.normals_f32_device(_dev(vol).data_ptr(), nelts, dims, blur, out.data_ptr())
    got = out.cpu().numpy()
    if min(dims) >= 12:
        c = (nz // 2, ny // 2, nx // 2)
        assert (ref[c[0], c[1], c[2] + 1] == 128).all()                    # beside the NaN
        assert blur or (ref[3:6, 4:7, 3:7] == 128).all()                   # inside the flat patch
    assert np.array_equal(got, ref), "differs in %d voxels" % int((got != ref).any(-1).sum())


@functools.lru_cache(maxsize=None)
def merge_case(dims, nf):
    f = np.stack([smooth_field(dims, seed=e, plant=False) for e in range(nf)], axis=-1)
    if min(dims) >= 12:
        nx, ny, nz = dims
        f.view(np.uint32)[nz // 2, ny // 2, nx // 2, nf - 1] = 0x7fc12345     # one NaN voxel, with a payload
    ref, refn = P.merge_fields_f32(f)
    for a in (f, ref, refn):
        a.setflags(write=False)
    return f, ref, refn


@pytest.mark.parametrize("nf", [1, 2, 3])
@pytest.mark.parametrize("dims", SHAPES)
def test_merge_fields_f32_bit_exact(R, dims, nf):
    nx, ny, nz = dims
    f, ref, refn = merge_case(dims, nf)
    d = _dev(f)
    assert ref[..., nf].max() == 1.0 and np.isfinite(ref[..., nf]).all()
    for with_normals in (True, False):
        out = _zeros((nz, ny, nx, nf + 1), "float32")
        nrm = _zeros((nz, ny, nx, 3), "uint8")
        R.merge_fields_f32_device(d.data_ptr(), nf, dims, out.data_ptr(), nrm.data_ptr() if with_normals else None)
        got = out.cpu().numpy()
        assert np.array_equal(got[..., :nf].view(np.uint32), f.view(np.uint32))      # raw bits, the NaN's payload too
        assert np.array_equal(got[..., nf], ref[..., nf]), "G differs in %d voxels" % int((got[..., nf] != ref[..., nf]).sum())
        assert np.array_equal(nrm.cpu().numpy(), refn if with_normals else np.zeros_like(refn))


def test_merge_fields_f32_of_a_constant_volume(R):
    """maxm = 0: every G is 0 (not 0 / 0) and every normal the zero vector"""
    nx, ny, nz = 13, 9, 7
    f = np.full((nz, ny, nx, 2), 0.37, np.float32)
    f[..., 1] = -2.5
    out, nrm = _zeros((nz, ny, nx, 3), "float32"), _zeros((nz, ny, nx, 3), "uint8")
    out.fill_(9.0)
    R.merge_fields_f32_device(_dev(f).data_ptr(), 2, (nx, ny, nz), out.data_ptr(), nrm.data_ptr())
    ref, refn = P.merge_fields_f32(f)
    assert (ref[..., 2] == 0).all() and (refn == 128).all()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(nrm.cpu().numpy(), refn)


@pytest.mark.parametrize("nelts", [2, 3])
@pytest.mark.parametrize("dims", SHAPES)
def test_hist2d_f32_bit_exact(R, dims, nelts):
    nx, ny, nz = dims
    rng = np.random.default_rng(41)
    vol = (rng.random((nz, ny, nx, nelts)) * 1.2 - 0.1).astype(np.float32)
    flat = vol.reshape(-1, nelts)
    plants = np.array([np.nan, np.inf, -np.inf, 0.0, 1.0, 254.999 / 255], np.float32)
    flat[:6, 0] = plants
    flat[6:12, 1] = plants
    flat[12:18, :2] = plants[:, None]
    if min(dims) >= 12:
        vol[:4, :, :, :2] = (0.0312, 0.0)      # a uniform slab: whole waves in one bin
        vol[4:6, :, :, 0] = np.round(vol[4:6, :, :, 0] * 4) / 4     # few values: contended bins
    ref = P.hist2d_f32(vol)
    d = _dev(vol)
    got = R.hist2d_f32_device(d.data_ptr(), nelts, dims)
    assert ref.max() == 255 and np.count_nonzero(ref) > (1000 if min(dims) >= 12 else 1)
    assert np.array_equal(got, ref)
    # the u8 entry (pinned to the checker by test_gpu_prep.py) on the bytes b(.)
    b = np.stack([P.hist_bin(vol[..., 0]), P.hist_bin(vol[..., 1])], axis=-1)
    assert np.array_equal(got, R.hist2d_device(_dev(b).data_ptr(), 2, dims))


def test_hist2d_f32_of_a_float_aligned_pointer(R):
    """two-channel volume that starts one float into a buffer: 4-byte aligned, not 8 (no paired loads there)"""
    nx, ny, nz = dims = (21, 13, 9)
    rng = np.random.default_rng(43)
    vol = (rng.random((nz, ny, nx, 2)) * 1.2 - 0.1).astype(np.float32)
    vol[:3] = (0.5, 0.25)
    buf = _dev(np.concatenate([np.float32([9.0]), vol.ravel(), np.float32([9.0])]))
    assert (buf.data_ptr() + 4) % 8 == 4
    ref = P.hist2d_f32(vol)
    assert ref.max() == 255 and np.count_nonzero(ref) > 50
    assert np.array_equal(R.hist2d_f32_device(buf.data_ptr() + 4, 2, dims), ref)


def test_hist2d_f32_needs_two_channels(R):
    v = _dev(np.zeros((4, 4, 4, 1), np.float32))
    with pytest.raises(Exception, match="not implemented"):
        R.hist2d_f32_device(v.data_ptr(), 1, (4, 4, 4))


def test_bad_arguments_are_refused_and_the_context_still_renders(R, smk):
    dims = (8, 7, 6)
    f = _dev(np.zeros((6, 7, 8, 3), np.float32))
    out, nrm = _zeros((6, 7, 8, 4), "float32"), _zeros((6, 7, 8, 3), "uint8")
    bad = [
        lambda: R.normals_f32_device(None, 1, dims, 0, nrm.data_ptr()),
        lambda: R.normals_f32_device(f.data_ptr(), 1, dims, 0, None),
        lambda: R.merge_fields_f32_device(None, 1, dims, out.data_ptr(), None),
        lambda: R.merge_fields_f32_device(f.data_ptr(), 1, dims, None, nrm.data_ptr()),
        lambda: R.merge_fields_f32_device(f.data_ptr(), 4, dims, out.data_ptr(), None),
        lambda: R.merge_fields_f32_device(f.data_ptr(), 0, dims, out.data_ptr(), None),
        lambda: R.merge_fields_f32_device(f.data_ptr(), 1, (8, 7, 2), out.data_ptr(), None),
        lambda: R.merge_fields_f32_device(f.data_ptr(), 1, (2, 7, 6), out.data_ptr(), None),
        lambda: R.hist2d_f32_device(None, 2, dims),
    ]
    for call in bad:
        with pytest.raises(smk.SmkError, match=r"smk_\w+_f32_device: \w+"):
            call()
    assert not out.any() and not nrm.any()
    sc = make_scene("cfg3", f32=True, shade=1)
    push_scene(R, sc)
    assert np.abs(R.render() - sc.render()).max() <= 1e-4


def test_float_chain_end_to_end(R, O):
    """merge_fields_f32_device (one field, with normals) -> upload_volume_device -> a shaded frame: the gather and the
    slice-ring kernel agree bit for bit on the uploaded floats, and both are within the project's parity bound (1e-4)
    of the checker rendering the restatement's arrays"""
    nx, ny, nz = dims = (24, 20, 18)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    r = np.sqrt(((x + .5) / nx - .5) ** 2 + ((y + .5) / ny - .5) ** 2 + ((z + .5) / nz - .5) ** 2)
    v = (0.45 + 0.4 * np.cos(11 * r) * np.exp(-2 * r) + 0.05 * np.sin(x * .7 + y * .45)).astype(np.float32)[..., None]
    assert np.abs(v * 255 - np.round(v * 255)).min() > 0
    ref_merged, ref_normals = P.merge_fields_f32(v)
    out, nrm = _zeros((nz, ny, nx, 2), "float32"), _zeros((nz, ny, nx, 3), "uint8")
    R.merge_fields_f32_device(_dev(v).data_ptr(), 1, dims, out.data_ptr(), nrm.data_ptr())
    assert np.array_equal(out.cpu().numpy(), ref_merged) and np.array_equal(nrm.cpu().numpy(), ref_normals)

    sc = O.Scene(ref_merged, grad=ref_normals)
    sc.tf_mode, sc.tf_vg = 1, tf_cfg3()
    sc.width = sc.height = 48
    sc.steps = 48
    sc.xform = O.rotation((1, 1, 0), 30)
    sc.shade_mode, sc.use_spec = 1, 1          # R8k diffuse + specular
    want = sc.render()
    assert want[..., 3].max() > 0.05
    R.upload_volume_device(out.data_ptr(), dims, 2, 1, nrm.data_ptr(), fsize=tuple(float(f) for f in sc.fsize), dmode="V1G")
    push_scene(R, sc, upload=False)
    frames = {}
    try:
        for kernel in (1, 2):
            R.set_option("kernel", kernel)
            frames[kernel] = R.render()
            assert R.last_frame_info()[0] == kernel
    finally:
        R.set_option("kernel", 0)
    assert np.array_equal(frames[1], frames[2])
    for kernel in (1, 2):
        assert np.abs(frames[kernel] - want).max() <= 1e-4, kernel
