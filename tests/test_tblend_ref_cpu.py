"""Qualifies the cases of tests/test_gpu_tblend.py without a GPU: the NumPy restatement of smk_blend_timesteps
(tests/_tblend_ref.py) has exact endpoints and stays in range, it differs from the three implementations the contract
excludes -- x + w (y - x), a blend in double rounded once, a contracted fma -- on the very volumes and at the very weights
the GPU tests use, and a frame of a blended step differs visibly from the frames of both end steps."""
import numpy as np
import pytest

import _tblend_ref as T
from _u16_ref import q8

DTYPES = ("u8", "f32", "u16")


def fields(dtype, seed, dims=None):
    """(x of every stored field of step `seed`, top) pairs"""
    data, grad = T.step(dtype, seed, dims)
    if dtype == "u8":
        return [(data, 255), (grad, 255)]
    if dtype == "f32":
        return [(data, None), (grad, 255)]
    return [(data[..., :2], 65535), (q8(data[..., 2]), 255), (grad, 255)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_endpoints_are_exact_and_integers_stay_in_range(dtype):
    a, b = T.step(dtype, 1), T.step(dtype, 2)
    d0, g0 = T.blend(a[0], a[1], b[0], b[1], 0.0)
    d1, g1 = T.blend(a[0], a[1], b[0], b[1], 1.0)
    assert np.array_equal(g0, a[1]) and np.array_equal(g1, b[1])
    if dtype == "u16":                 # (the third channel comes back as its stored byte)
        for d, s in ((d0, a[0]), (d1, b[0])):
            assert np.array_equal(d[..., :2], s[..., :2]) and np.array_equal(q8(d[..., 2]), q8(s[..., 2]))
    else:
        assert np.array_equal(d0, a[0]) and np.array_equal(d1, b[0])
    if dtype != "f32":
        top = 255 if dtype == "u8" else 65535
        hi = np.full((4, 4, 4, 3), top, a[0].dtype)
        for w in (0.0, 0.3, 0.5, 0.7, 1.0 / 3.0, 1.0):
            d, g = T.blend(hi, hi[..., :3].astype(np.uint8), hi, hi[..., :3].astype(np.uint8), w)
            assert d.dtype == a[0].dtype and int(d.max()) <= top and int(d[..., :2].min()) == top and np.all(g == 255)


def test_the_u16_third_channel_survives_the_round_trip():
    b = np.arange(256, dtype=np.uint32)
    assert np.array_equal(q8(b * 257), b)


def test_a_missing_normal_stays_put():
    n = np.full(8, 128, np.uint8)
    for w in np.linspace(0, 1, 1001).astype(np.float32):
        assert np.all(T.right(n, n, w, 255) == 128)
    assert np.all(T.right(n * 0, n * 0, 0.3, 255) == 0)          # (the pad column of an odd-sized 8-byte-voxel volume)


@pytest.mark.parametrize("w, lerp, f64", [(0.3, 143, 3133), (0.7, 143, 3133), (0.25, 0, 0), (0.5, 0, 0), (1.0 / 3.0, 0, 0)])
def test_exhaustive_byte_pairs(w, lerp, f64):
    """why the GPU tests blend at 0.3 and 0.7: of the 65536 byte pairs these many tell the formulas apart"""
    x, y = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    r = T.right(x, y, w, 255)
    assert int((r != T.wrong_lerp(x, y, w, 255)).sum()) == lerp
    assert int((r != T.wrong_f64(x, y, w, 255)).sum()) == f64


def test_random_floats_tell_the_float_formulas_apart():
    """why the f32 cases add w = 1/3: of 2^20 pairs of normally distributed floats about half differ from x + w (y - x)
    and about a third from the contracted form (measured 0.51 and 0.30)"""
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal(1 << 20, np.float32), rng.standard_normal(1 << 20, np.float32)
    r = T.right(x, y, 1.0 / 3.0)
    assert 0.4 < (r != T.wrong_lerp(x, y, 1.0 / 3.0)).mean() < 0.6
    assert 0.2 < (r != T.wrong_fma(x, y, 1.0 / 3.0)).mean() < 0.4


# differences between the restatement and each wrong formula, summed over the stored fields of steps 1 and 2, as counted
# when the cases were chosen: {(dtype, dims, w): (x + w (y - x), double rounded once, contracted fma)}.  Recorded, so that a
# change of a generator cannot take a thin one (u16 against the first form: one voxel) to zero unnoticed
ODD = (31, 29, 27)
COUNTS = {
    ("u8", None, 0.3): (80, 3884, 80), ("u8", None, 0.7): (89, 4299, 98),
    ("f32", None, 0.3): (6654, 8066, 5410), ("f32", None, 0.7): (10069, 7534, 3740), ("f32", None, 1.0 / 3.0): (11904, 12712, 5118),
    ("u16", None, 0.3): (1, 9272, 1), ("u16", None, 0.7): (0, 8101, 3),
    ("u8", ODD, 0.3): (3, 5855, 3), ("u16", ODD, 0.3): (1, 6860, 1),      # (the layout cases' all-odd volumes, blended at 0.3)
}


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_wrong_formulas_show_on_the_test_volumes(dtype):
    """every wrong formula -- the contracted one on the integer types too -- shows on some voxel of the volumes the GPU cases
    of this type blend, at one of their weights"""
    total = [0, 0, 0]
    for (dt, dims, w), want in COUNTS.items():
        if dt != dtype:
            continue
        n = [0, 0, 0]
        for (x, top), (y, _) in zip(fields(dtype, 1, dims), fields(dtype, 2, dims)):
            r = T.right(x, y, w, top)
            for k, f in enumerate((T.wrong_lerp, T.wrong_f64, T.wrong_fma)):
                n[k] += int((r != f(x, y, w, top)).sum())
        print("\n", dtype, dims, w, n)
        assert tuple(n) == want, (dtype, dims, w, n)
        if dims is None:
            total = [a + b for a, b in zip(total, n)]
    assert all(t > 0 for t in total), total


def test_the_blended_frame_is_neither_end_frame():
    """a GPU test that showed step a or step b instead of the blend would fail: the checker's frames differ by far more
    than any tolerance in use"""
    a, b = T.step("f32", 1), T.step("f32", 2)
    m = T.blended("f32", 1, 2, 0.3)
    fa, fb, fm = (T.scene(*s).render() for s in (a, b, m))
    assert np.abs(fm - fa).max() > 1e-3 and np.abs(fm - fb).max() > 1e-3
