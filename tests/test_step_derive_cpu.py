"""The volumes of tests/test_gpu_step_derive.py, qualified on the CPU checker (tests/_step_derive_ref.py): every property a
wrong derive could hide behind must show on them, so that no GPU test can pass vacuously.  No GPU."""
import numpy as np
import pytest

import _step_derive_ref as R
import _tblend_ref as T


@pytest.mark.parametrize("ring", R.RINGS)
@pytest.mark.parametrize("dims", R.DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_the_blend_of_steps_0_and_1_shows_every_trap(O, dims, ring):
    a, b, (mixed, _) = R.blended(O, dims, ring)
    s = np.ascontiguousarray(mixed[..., 0])                 # the blended SCALAR: the stored channel 0
    assert s.dtype == R.NP[ring] and s.shape == dims[::-1]
    # interior voxels with zero gradient exist: H is NaN there
    f = s.astype(np.float64)
    gx, gy, gz = f[1:-1, 1:-1, 2:] - f[1:-1, 1:-1, :-2], f[1:-1, 2:, 1:-1] - f[1:-1, :-2, 1:-1], f[2:, 1:-1, 1:-1] - f[:-2, 1:-1, 1:-1]
    flat = int(((gx == 0) & (gy == 0) & (gz == 0)).sum())
    assert flat >= 36, flat                                 # (the inside of the flat block)
    want, wnrm = R.derive(O, s, ring, 1, 0)
    if ring == "f32":                                       # ... and the float H of those voxels is the contract's 0
        assert np.isfinite(want).all()
    # G and H of the blended scalar are not the blended G and H
    differ = int((R.downloaded(want, wnrm)[0][..., 1:] != R.downloaded(mixed, wnrm)[0][..., 1:]).sum())
    assert differ > want[..., 1:].size // 4, differ
    print("%s %s: zero-gradient voxels %d, G/H values differing %d" % (dims, ring, flat, differ))
    # V is rescaled: channel 0 of the output is not a copy of the source
    assert not np.array_equal(want[..., 0], s)
    # the 1-voxel border is 0 in all three channels
    inner = np.zeros(s.shape, bool)
    inner[1:-1, 1:-1, 1:-1] = True
    assert not want[~inner].any() and want[inner][..., 0].any()
    # compat 0 and 1 differ (in H alone)
    other = R.derive(O, s, ring, 0, 0)[0]
    assert not np.array_equal(other[..., 2], want[..., 2]) and np.array_equal(other[..., :2], want[..., :2])
    # blurred and plain normals differ, on the border too (a blurred border voxel gathers its interior neighbours)
    blur = R.derive(O, s, ring, 1, 1)[1]
    assert not np.array_equal(blur, wnrm)
    assert (wnrm[~inner] == 128).all() and not (blur[~inner] == 128).all()
    # the normals' source is the OUTPUT V channel: those of the input scalar are others
    if ring == "u8":
        assert not np.array_equal(O.normals_vgh(np.ascontiguousarray(mixed), blur=False), wnrm)


def test_the_issues_figures_for_the_u8_series(O):
    """36 zero-gradient voxels for both sizes; 42 465 and 6 714 G/H bytes between the derived and the blended step"""
    for dims, nbytes in zip(R.DIMS, (42465, 6714)):
        _, _, (mixed, _) = R.blended(O, dims, "u8")
        s = mixed[..., 0].astype(np.int32)
        g0 = (s[1:-1, 1:-1, 2:] == s[1:-1, 1:-1, :-2]) & (s[1:-1, 2:, 1:-1] == s[1:-1, :-2, 1:-1]) & (s[2:, 1:-1, 1:-1] == s[:-2, 1:-1, 1:-1])
        want = R.derive(O, np.ascontiguousarray(mixed[..., 0]), "u8")[0]
        assert (int(g0.sum()), int((want[..., 1:] != mixed[..., 1:]).sum())) == (36, nbytes)


def test_the_typed_scalars_keep_the_structure():
    v = R.scalar(0, R.SMALL)
    for kind in R.RINGS:
        s = R.as_type(v, kind)
        assert s.dtype == R.NP[kind] and s.shape == v.shape
        assert len(np.unique(s[2:7, 3:8, 4:10])) == 1      # the flat block stays flat
        assert len(np.unique(s)) > 100


def test_the_blend_is_tblends(O):
    a, b, m = R.blended(O, R.SMALL, "u16")
    w = T.blend(a[0], a[1], b[0], b[1], R.W)
    assert np.array_equal(m[0], w[0]) and np.array_equal(m[1], w[1])
