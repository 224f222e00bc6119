"""SMK_U16 voxels without a GPU: the layout's 8-bit third channel, the float -> u16 rule, the 16-bit load of the host-side
volume files (simian-spacemonkey_amd/host/VolumeFiles.cpp, driven through tests/host/files16_main), and the qualification
of the cases tests/test_gpu_u16.py renders -- above all that its fine-structure scene cannot be passed by a build that
quietly fell back to 8 bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "files16_main")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import volume_files as VF  # noqa: E402

import _u16_ref as U  # noqa: E402


# ------------------------------------------------------------------------------------------------ the layout

def test_q8_over_all_inputs():
    c = np.arange(65536)
    q = U.q8(c).astype(np.int64)
    assert q[0] == 0 and q[65535] == 255
    assert (np.diff(q) >= 0).all() and set(np.unique(q)) == set(range(256))
    # within half a step of c * 255 / 65535: |q * 65535 - c * 255| <= 65535 / 2, in integers
    assert (np.abs(q * 65535 - c * 255) * 2 <= 65535).all()
    # the 8-bit unorms themselves, widened exactly (v * 257), come back
    assert np.array_equal(U.q8(np.arange(256) * 257), np.arange(256))


def test_pack_and_decode():
    rng = np.random.default_rng(2)
    d = rng.integers(0, 65536, (3, 4, 5, 3), dtype=np.uint16)
    g = rng.integers(0, 256, (3, 4, 5, 3), dtype=np.uint8)
    p = U.pack_u16(d, g)
    assert p.dtype == np.uint32 and p.shape == (3, 4, 5, 2)
    assert np.array_equal(p[..., 0] & 0xffff, d[..., 0]) and np.array_equal(p[..., 0] >> 16, d[..., 1])
    for k in range(3):      # the normal bytes sit where the u8 voxel has them
        assert np.array_equal((p[..., 1] >> (8 * k)) & 0xff, g[..., k])
    assert np.array_equal(p[..., 1] >> 24, U.q8(d[..., 2]))
    one = U.pack_u16(d[..., :1])
    assert np.array_equal(one[..., 0], d[..., 0]) and (one[..., 1] == 0x808080).all()      # missing channels 0, no normals
    f = U.decode_u16(d)
    assert f.dtype == np.float32 and f.min() >= 0 and f.max() <= 1
    assert np.array_equal(f[..., 0], d[..., 0].astype(np.float32) / np.float32(65535))
    assert np.array_equal(f[..., 2], U.q8(d[..., 2]).astype(np.float32) / np.float32(255))
    assert U.decode_u16(np.array([[65535, 65535, 65535]], np.uint16)).tolist() == [[1.0, 1.0, 1.0]]


def test_quantize_u16_edge_cases():
    f = np.float32
    v = np.array([np.nan, np.inf, -np.inf, -1.0, -1e-30, -0.0, 0.0, 1.0, 1.5, 0.5, 1.5 / 65535, 2.5 / 65535, 0.49 / 65535,
                  np.nextafter(f(1), f(0)), 65534.4 / 65535, 3e38, 1e-45], np.float32)
    want = [0, 65535, 0, 0, 0, 0, 0, 65535, 65535, 32768, 2, 3, 0, 65535, 65534, 65535, 0]
    assert U.quantize_u16(v).tolist() == want
    # exact halves round up (one fp32 add, then truncation): t = k + .5 is exact in float32 for these v
    for k in (1, 2, 7, 100, 4095):
        v = np.float32((k + .5) / 65535.0)
        if np.float32(v * np.float32(65535.0)) == np.float32(k + .5):
            assert U.quantize_u16(v) == k + 1
    # every code point is a fixed point of decode -> quantise
    c = np.arange(65536).astype(np.uint16)
    assert np.array_equal(U.quantize_u16(U.decode_u16(c[:, None])[:, 0]), c)


# ------------------------------------------------------------------------------------------------ the 16-bit load

def test_driver_is_built():
    assert os.path.exists(EXE), "build with __graft_entry__.build()"


def quantize16(native):
    return U.quantize_file16(native).ravel()


def _trex(tmp_path, raw, dims, tname, endian):
    nx, ny, nz = dims
    trex = tmp_path / "vol.trex"
    trex.write_text("# typed brick\nData Set Name: t\nData Set Files:   %s\nNumber of Time Steps: 1, 0, 0\n"
                    "Volume Size int: %d, %d, %d\nVolume Size float: 1, 1, 1\nDon't append numbers\n"
                    "Data Type: %s\nEndian: %s\nNumber of Sub Volumes: 1\nSubVolume {\n  Size int: %d, %d, %d\n"
                    "  Size float: 1, 1, 1\n  Pos int: 0, 0, 0\n  Pos float: 0, 0, 0\n}\n"
                    % (raw, nx, ny, nz, tname, endian, nx, ny, nz))
    return trex


def _load16(tmp_path, trex):
    o16, o8 = tmp_path / "out.u16", tmp_path / "out.u8"
    p = subprocess.run([EXE, "load16", str(trex), "0", str(o16), str(o8)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    kv = dict(line.split("=", 1) for line in p.stdout.splitlines())
    return kv, np.fromfile(o16, np.uint16), np.fromfile(o8, np.uint8)


@pytest.mark.parametrize("tname,dtype", [("float", "f4"), ("short", "i2"), ("ushort", "u2"), ("int", "i4"),
                                         ("uint", "u4"), ("uchar", "u1"), ("double", "f8")])
@pytest.mark.parametrize("endian", ["big", "little"])
def test_typed_raw_bricks_load_as_16_bits(tmp_path, tname, dtype, endian):
    rng = np.random.default_rng(11)
    dims = (9, 7, 5)
    nx, ny, nz = dims
    if dtype.startswith("f"):
        native = (rng.normal(size=(nz, ny, nx)) * 37.5 + 3).astype(dtype)
    else:
        info = np.iinfo(dtype)
        native = rng.integers(max(info.min, -30000), min(info.max, 60000), size=(nz, ny, nx)).astype(dtype)
    raw = tmp_path / "vol"
    native.astype(np.dtype(dtype).newbyteorder(">" if endian == "big" else "<")).tofile(raw)
    trex = _trex(tmp_path, raw, dims, tname, endian)
    kv, got16, got8 = _load16(tmp_path, trex)
    assert kv["bytes"] == str(native.nbytes) and kv["bricks16"] == "1" and kv["points16"] == "1"
    if dtype == "u1":
        want = native.ravel().astype(np.uint16) * 257        # (bytes are widened as unorms)
    else:
        want = quantize16(native)
        assert got16.min() == 0 and got16.max() == 65535     # min/max quantisation spans the 16-bit range
        assert len(np.unique(got16)) > 256 or native.size <= 256 or len(np.unique(native)) <= 256
    assert np.array_equal(got16, want)
    # the 8-bit voxels of the same load are the reference path's, unchanged
    h = VF.parse_trex(trex.read_text())
    want8 = VF.read_raw_brick(h, str(raw), 0) if dtype != "f8" else VF.quantize(native.astype(np.float64).ravel())
    assert np.array_equal(got8, want8.ravel())


def test_constant_volume_loads_as_zero(tmp_path):
    raw = tmp_path / "c"
    np.full(27, 4.5, np.float32).tofile(raw)
    kv, got16, got8 = _load16(tmp_path, _trex(tmp_path, raw, (3, 3, 3), "float", "little"))
    assert not got16.any() and not got8.any() and got16.size == 27


# ------------------------------------------------------------------------------------------------ the GPU cases, qualified

def test_volumes_use_all_sixteen_bits():
    for dims in (U.DIMS_EVEN, U.DIMS_ODD, U.DIMS_33):
        d, nrm = U.volume16(dims)
        assert d.dtype == np.uint16 and d.shape == dims[::-1] + (3,) and nrm.shape == d.shape
        assert d[..., 0].min() == 0 and d[..., 0].max() == 65535
        for e in range(2):      # (the channels stored whole) an 8-bit volume widened to 16 bits would have 256 distinct values
            assert len(np.unique(d[..., e])) > 2000, e
    assert all(n & 1 for n in U.DIMS_ODD) and not U.DIMS_EVEN[0] & 1


def test_brick_cuts_tile_the_odd_volume():
    d, _ = U.volume16(U.DIMS_ODD)
    fs = U.case(3, dims=U.DIMS_ODD).sc.fsize
    for grid in sorted(U.CUTS):
        bs = U.bricks(U.DIMS_ODD, fs, grid)
        assert len(bs) == grid[0] * grid[1] * grid[2]
        assert sum(b[1][0] * b[1][1] * b[1][2] for b in bs) == d[..., 0].size
        sizes = {b[1] for b in bs}
        assert len(sizes) > 1, "the bricks are all the same size"
        for a in range(3):      # the extent the single brick states, exactly
            assert max(np.float32(np.float32(b[2][a]) + np.float32(b[3][a])) for b in bs) == np.float32(fs[a])


@pytest.mark.parametrize("c", U.PARITY, ids=U.parity_id)
def test_parity_cases_show_something(c):
    k = U.parity_case(c)
    ref = k.sc.render(blend=c[4])
    assert ref[..., 3].max() > 0.05 and np.isfinite(ref).all()
    if k.sc.tf_mode == 0:
        assert k.sc.tlut.shape == (256, 4)          # (the 1-D tables of the parity cases: 256 entries, _u16_ref.table_1d)
    if c[5]:                                        # first-hit depth only under tables without a transparent texel
        assert k.sc.tf_vg[..., 3].min() > 0 and (k.sc.tf_h is None or k.sc.tf_h[..., 3].min() > 0)


def test_parity_cases_cover_what_they_claim():
    P = U.PARITY
    assert {c[0] for c in P} == {1, 2, 3} and {c[1] for c in P} == {"1d", "2d", "2d3", "3d"}
    assert {c[2] for c in P} == {0, 1, 2} and {c[4] for c in P} == {0, 1, 2} and any(c[5] for c in P)
    assert {c[3][0] for c in P} >= {"x", "y", "z"}
    assert U.parity_case([c for c in P if c[1] == "2d3"][0]).sc.third_axis == 1


def test_fine_structure_is_lost_at_eight_bits():
    """the qualification of test_gpu_u16.py's fine-structure test: the checker's frame of the decoded u16 volume and its
    frame of the same voxels quantised to 8 bits differ by at least 100 x the parity tolerance"""
    d = U.fine_volume()
    v = d[..., 0].astype(np.float64) / 65535.0
    ramp = v.mean(axis=(0, 1))
    assert (np.diff(ramp) > 0).all()                                  # a smooth ramp along x ...
    detail = v - ramp[None, None, :]
    assert 0.2 / 255 < np.abs(detail).max() < 0.5 / 255               # ... plus detail below one 8-bit step
    t = U.fine_table()
    a = t[0, :, 3].astype(int)
    assert (t[..., 3] == t[:1, :, 3]).all() and a[127] == 0 and a[129] == 255 and 0 < a[128] < 255 and (np.diff(a) >= 0).all()
    f16 = U.fine_case().sc.render()
    f8 = U.fine_case(eight_bit=True).sc.render()
    assert f16[..., 3].max() > 0.05
    diff = np.abs(f16 - f8).max()
    assert diff >= 100 * U.TOL and diff >= 1e-2, diff
