"""The volumes of tests/test_gpu_step_derive.py, tests/test_gpu_step_derive_shapes.py and the float and second-grid-turn cases
of tests/test_gpu_prep.py, qualified on the CPU checker (tests/_step_derive_ref.py): every property a wrong derive could
hide behind must show on them, so that no GPU test can pass vacuously.  No GPU."""
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


# ---- the volumes of tests/test_gpu_step_derive_shapes.py and of the float cases of tests/test_gpu_prep.py

def inner(a):
    return a[1:-1, 1:-1, 1:-1]


@pytest.mark.parametrize("dims", [R.SMALL, (5, 4, 3)], ids=lambda d: "%dx%dx%d" % d)
def test_the_float_scalars_leave_the_unit_range_and_meet_the_seeds(O, dims):
    v8 = R.scalar(0, dims) if dims == R.SMALL else R.small_scalar(dims)
    seen = {}
    for name in R.SCALARS:
        s = R.typed(v8, name)
        assert s.dtype == R.NP[R.KIND[name]] and s.shape == dims[::-1] and np.isfinite(s.astype(np.float64)).all()
        v8o, vf = O.make_vgh(s if s.dtype == np.uint8 else s.astype(np.float32), compat=True, f32=True)
        assert np.isfinite(vf).all(), name
        # a zero-gradient interior voxel: G is 0 there, and its NaN H is stored as 0
        flat = inner(vf[..., 1]) == 0
        assert flat.any() and not inner(vf[..., 2])[flat].any(), name
        assert not np.array_equal(O.make_vgh(s if s.dtype == np.uint8 else s.astype(np.float32), compat=False, f32=True)[1], vf), name
        seen[name] = (float(s.min()), float(s.max()), float(inner(vf[..., 0]).min()), float(inner(vf[..., 0]).max()))
        print(dims, name, "scalar %g .. %g, interior V %g .. %g" % seen[name])
    lo, hi, vlo, vhi = seen["signed"]
    assert lo < -2 and hi > 10 and (vlo, vhi) == (0.0, 1.0)          # both signs; the observed extremes scale V
    s = R.typed(v8, "signed")
    z = R.minus_zero_at(s.shape)
    assert s.view(np.uint32)[z] == 0x80000000 and (s.view(np.uint32) == 0x80000000).sum() == 1
    assert 0 < z[0] < s.shape[0] - 1 and 0 < z[1] < s.shape[1] - 1 and 0 < z[2] < s.shape[2] - 1
    lo, hi, vlo, vhi = seen["above"]
    assert lo > 1e8 and vlo > 0.02 and vhi == 1.0                    # the seed 1e8 is dmin: no interior V is 0
    lo, hi, vlo, vhi = seen["below"]
    assert hi < -1e8 and vlo == 0.0 and vhi < 0.98                   # the seed -1e8 is dmax: no interior V is 1
    if dims == R.SMALL:                                              # (the issue's figures)
        assert abs(seen["signed"][0] + 2.74) < .01 and abs(seen["signed"][1] - 11.39) < .01
        assert abs(seen["above"][2] - 0.0616) < 1e-4 and abs(seen["below"][3] - 0.938) < 1e-3


def test_the_tile_shapes_cover_every_edge():
    xs, ys, zs = (set(d[a] for d in R.TILE_SHAPES) for a in range(3))
    assert xs >= {31, 32, 33, 34, 63, 64, 65} and ys >= {7, 8, 9, 10, 16, 17} and zs >= {8, 9, 10, 17}
    assert (32, 8, 8) in R.TILE_SHAPES and (64, 16, 8) in R.TILE_SHAPES
    assert R.TILE == (32, 8, 8) and len(R.TILE_SHAPES) <= 12


@pytest.mark.parametrize("ring", R.RINGS)
@pytest.mark.parametrize("dims", R.TILE_SHAPES, ids=lambda d: "%dx%dx%d" % d)
def test_blur_shows_in_the_last_tile_of_every_axis(O, dims, ring):
    """blurred and plain normals of the noise differ among the voxels of the last tile in x, in y, in z, and in the tile that
    is last on all three -- a tile that holds border voxels only included: a blurred border voxel gathers its neighbours"""
    s = R.typed(R.noise(dims), ring)
    assert len(np.unique(R.noise(dims))) > 250
    (d0, n0), (d1, n1) = (R.derive(O, s, ring, 1, blur) for blur in (0, 1))
    assert np.array_equal(d0, d1) and inner(d0).any(axis=(0, 1, 2)).all()
    zl, yl, xl = R.last_tile(dims)
    for what, region in (("x", (slice(None), slice(None), xl)), ("y", (slice(None), yl, slice(None))),
                         ("z", (zl, slice(None), slice(None))), ("corner", (zl, yl, xl))):
        assert n0[region].size and not np.array_equal(n0[region], n1[region]), what


def test_the_thin_volume_needs_the_second_turn_of_the_stats_loop(O):
    """what the stats pass would make of THIN if every workgroup stopped after its first tile: the extremes of z < 344
    alone.  They differ from the whole volume's, and the checker's output of that slab differs from its output of the whole
    volume in more than half of the bytes of each channel of the first-turn voxels"""
    nx, ny, nz = R.THIN
    gx, gy, gz = ((n + t - 1) // t for n, t in zip(R.THIN, R.TILE))
    assert (gx, gy, gz) == (1, 48, 46) and gx * gy * gz - R.STATS_BLOCKS == 160
    first = [(t % gx, (t // gx) % gy, t // (gx * gy)) for t in range(R.STATS_BLOCKS)]
    assert (max(b[2] for b in first) + 1) * R.TILE[2] == R.SECOND_TURN_Z   # no first-turn tile reaches z >= 344
    s = R.thin_scalar()
    assert (int((s == 0).sum()), int((s == 255).sum())) == (1, 1) and s[R.PLANT[0]] == 0 and s[R.PLANT[1]] == 255
    assert all(p[0] >= 350 and 0 < p[1] < ny - 1 and 0 < p[2] < nx - 1 for p in R.PLANT)
    assert sum(abs(a - b) for a, b in zip(*R.PLANT)) == 1
    head = inner(s[:R.SECOND_TURN_Z + 1])                            # the interior voxels of z < 344
    assert 40 <= int(head.min()) and int(head.max()) <= 215 and (int(inner(s).min()), int(inner(s).max())) == (0, 255)
    print("interior extremes: %d .. %d for z < 344, 0 .. 255 for the whole" % (head.min(), head.max()))
    for compat in (0, 1):
        whole = O.make_vgh(s, compat=bool(compat))
        slab = O.make_vgh(np.ascontiguousarray(s[:R.SECOND_TURN_Z + 1]), compat=bool(compat))
        for c, name in enumerate("VGH"):
            a, b = inner(whole[:R.SECOND_TURN_Z + 1])[..., c], inner(slab)[..., c]
            frac = float((a != b).mean())
            print("compat %d, %s: %.1f %% of the first-turn bytes change" % (compat, name, 100 * frac))
            assert frac > 0.5, (compat, name, frac)
    for kind in ("u8", "f32"):                                       # the typed scalars keep the extremes where they are
        t = R.as_type(s, kind)
        assert np.unravel_index(int(np.argmin(t)), t.shape) == R.PLANT[0] and np.unravel_index(int(np.argmax(t)), t.shape) == R.PLANT[1]


def test_the_big_volume_needs_a_second_grid_turn(O):
    """BIG's interior extremes lie where only a second turn of smk_make_vgh_device's grid reads them; what lies beyond the
    normals grid is border, whose blurred normals are not the zero vector"""
    s = R.big_scalar()
    nx, ny, nz = R.BIG
    assert s.shape == (nz, ny, nx) and s.size > R.NRM_THREADS and s.size > 2 * R.VGH_THREADS
    assert R.linear(R.BIG_MIN, R.BIG) > R.VGH_THREADS and R.linear(R.BIG_MAX, R.BIG) > R.VGH_THREADS
    assert R.linear((nz - 2, ny - 2, nx - 2), R.BIG) < 2 * R.VGH_THREADS       # no interior voxel lies in a third turn
    first = s.reshape(-1)[:R.VGH_THREADS]
    assert (int(inner(s).min()), int(inner(s).max())) == (5, 250) == (int(s[R.BIG_MIN]), int(s[R.BIG_MAX]))
    assert 40 <= int(first.min()) and int(first.max()) <= 215     # what a single turn sees
    tail = s.reshape(-1)[2 * R.VGH_THREADS:]
    assert (int(s.min()), int(s.max())) == (0, 255) == (int(tail.min()), int(tail.max()))
    vgh = O.make_vgh(s)
    plain, blurred = (O.normals_vgh(vgh, blur=b).reshape(-1, 3)[R.NRM_THREADS:] for b in (False, True))
    assert (plain == 128).all() and (blurred != 128).any(axis=1).mean() > 0.9
