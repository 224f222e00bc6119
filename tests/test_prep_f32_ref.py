"""tests/_prep_f32_ref.py, the float32 restatement the GPU float-prep tests compare with, against the
reference-derived checker (oracle/smk_prep.c): on byte data widened to float the float contracts must give the bytes
the u8 arithmetic gives, so tests/test_gpu_prep_f32.py is not product against product.  No GPU."""
import numpy as np
import pytest

import _prep_f32_ref as P
from _scenes import ragged_vgh, scalar_volume


def _byte_volumes():
    return {"spheres32": np.ascontiguousarray(scalar_volume(32, 1)[..., None]), "ragged": ragged_vgh()[0]}


@pytest.fixture(scope="module")
def byte_volumes():
    return _byte_volumes()


@pytest.mark.parametrize("blur", [False, True])
@pytest.mark.parametrize("name", ["spheres32", "ragged"])
def test_normals_of_widened_bytes_equal_the_checker(O, byte_volumes, name, blur):
    v8 = byte_volumes[name]
    ref = O.normals_vgh(v8, blur=blur)
    assert len(np.unique(ref.reshape(-1, 3), axis=0)) > 50
    assert np.array_equal(P.normals_f32(v8.astype(np.float32), blur=blur), ref)


@pytest.mark.parametrize("name", ["spheres32", "ragged"])
def test_merge_of_widened_bytes_equals_the_checker(O, byte_volumes, name):
    v8 = byte_volumes[name]
    ref, refn = O.merge_addg(v8)
    nf = v8.shape[-1]
    out, nrm = P.merge_fields_f32(v8.astype(np.float32))
    assert out.dtype == np.float32 and out.shape == ref.shape
    assert np.array_equal(out[..., :nf], v8.astype(np.float32))
    assert ref[..., nf].max() == 255 and out[..., nf].max() == 1.0
    assert np.array_equal(np.trunc(out[..., nf].astype(np.float64) * 255.0).astype(np.uint8), ref[..., nf])
    assert np.array_equal(nrm, refn)


def test_histogram_of_bin_centres_equals_the_checker(O, byte_volumes):
    v8 = byte_volumes["ragged"]
    v = ((v8.astype(np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    assert np.array_equal(P.hist_bin(v), v8)
    ref = O.hist2d(v8)
    assert ref.max() == 255 and np.count_nonzero(ref) > 1000
    assert np.array_equal(P.hist2d_f32(v), ref)
    assert np.array_equal(P.hist2d_f32(v[..., :2]), ref)


def test_histogram_bins_at_the_edges():
    f = np.float32
    v = np.array([np.nan, -np.inf, -0.1, -0.0, 0.0, 1e-30, 1 / 255, 254.999 / 255, 1.0, 1.1, np.inf], f)
    assert P.hist_bin(v).tolist() == [0, 0, 0, 0, 0, 0, 1, 254, 255, 255, 255]
    below_one = np.nextafter(f(1), f(0))
    assert below_one * f(255) < f(255) and P.hist_bin(below_one) == 254


@pytest.mark.parametrize("blur", [False, True])
def test_normals_do_not_depend_on_the_scale(blur):
    """every step of the gradient scales exactly with a power of two, and the normalisation takes it out"""
    rng = np.random.default_rng(5)
    z, y, x = np.meshgrid(np.arange(14), np.arange(17), np.arange(19), indexing="ij")
    v = (0.5 + 0.3 * np.sin(x * .4) * np.cos(y * .3 + z * .2) + 0.1 * rng.random(x.shape)).astype(np.float32)[..., None]
    a, b = P.normals_f32(v, blur=blur), P.normals_f32(v * np.float32(2.0 ** -8), blur=blur)
    assert len(np.unique(a.reshape(-1, 3), axis=0)) > 100
    assert np.array_equal(a, b)


def test_a_shallow_ramp_keeps_its_normal_in_float_and_loses_it_in_bytes(O):
    """what the float entries are for: neighbours that differ by less than 1/255.  The float normals of a linear ramp
    are one direction everywhere inside; the byte copy's differences are 0 or 1, and somewhere all three are 0"""
    nx, ny, nz = 24, 20, 18
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = (0.3 + (x + 2 * y + 3 * z) / (8 * 255.0)).astype(np.float32)
    inner = P.normals_f32(v[..., None])[1:-1, 1:-1, 1:-1].reshape(-1, 3)
    assert (inner == inner[0]).all()
    # (1, 2, 3) / sqrt(14) through n * 128 + 128, truncated
    assert inner[0].tolist() == [int(128 + 128 * c / 14 ** .5) for c in (1, 2, 3)]
    v8 = np.floor(255.0 * v.astype(np.float64)).astype(np.uint8)
    inner8 = O.normals_vgh(np.ascontiguousarray(v8[..., None]))[1:-1, 1:-1, 1:-1].reshape(-1, 3)
    assert (inner8 == 128).all(axis=1).any()
    assert len(np.unique(inner8, axis=0)) > 1


def test_values_that_are_not_finite():
    """a NaN or infinite voxel zeroes the normals it reaches and never wins the maximum; a constant volume has G = 0"""
    rng = np.random.default_rng(9)
    v = rng.random((9, 10, 11, 2)).astype(np.float32)
    v[4, 5, 6, 0] = np.nan
    v[2, 3, 4, 1] = np.inf
    n = P.normals_f32(v)
    assert (n[4, 5, 5] == 128).all() and (n[4, 5, 7] == 128).all() and (n[3, 5, 6] == 128).all()
    assert not (n[4, 5, 6] == 128).all()          # (the centre is not part of its own central differences)
    out, nrm = P.merge_fields_f32(v)
    G = out[..., 2]
    assert np.isfinite(G).all() and G.max() == 1.0 and G.min() == 0.0
    assert G[4, 5, 5] == 0 and G[2, 3, 5] == 0 and (nrm[2, 3, 5] == 128).all()
    assert np.array_equal(out[..., :2].view(np.uint32), v.view(np.uint32))
    flat, nflat = P.merge_fields_f32(np.full((5, 4, 3, 1), 0.37, np.float32))
    assert (flat[..., 1] == 0).all() and (nflat == 128).all()
