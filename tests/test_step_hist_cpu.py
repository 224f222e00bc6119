"""The histogram and the probe of a resident time step without a GPU: the NumPy restatement (tests/_step_hist_ref.py)
against the checker, smk_hist2d_finish -- host-only, so the library runs it here -- against the restatement, the u16 bin
rule, the qualification of the cases tests/test_gpu_step_hist.py runs, and the header's five new declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _step_hist_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["smk_hist2d_step_device", "smk_hist2d_step", "smk_hist2d_finish", "smk_probe_step"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- the restatement against the checker

@pytest.mark.parametrize("nelts", [2, 3, 4])
def test_u8_restatement_equals_the_checker(O, nelts):
    data, _ = S.volume("u8", nelts)
    assert np.array_equal(S.finish(S.counts(data)), O.hist2d(data))
    # ... and on a box of it: the checker on the box's voxels
    g0, g1 = (20, 0, 22), (41, 18, 45)
    sub = np.ascontiguousarray(data[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]])
    assert np.array_equal(S.finish(S.counts(data, g0, g1)), O.hist2d(sub))


def test_f32_bins_on_byte_values_are_the_bytes():
    """v = b / 255 in fp32 need not bin as b; v = (b + 0.5) / 255 does, for every byte"""
    b = np.arange(256)
    assert np.array_equal(S.bin_f32(((b + 0.5) / 255.0).astype(np.float32)), b)


# ---- smk_hist2d_finish

def _finish(smk, counts):
    return smk.Renderer.hist2d_finish(counts)


def test_finish_known_answers(smk):
    """test_oracle_kat's: bins holding 1, 2, 8 and 64 voxels -> bytes 0, 42, 127, 255; empty bins 0"""
    c = np.zeros((256, 256), np.uint32)
    c[20, 10], c[20, 11], c[21, 12], c[3, 200] = 1, 2, 8, 64
    h = _finish(smk, c)
    assert (h[20, 10], h[20, 11], h[21, 12], h[3, 200]) == (0, 42, 127, 255)
    assert np.count_nonzero(h) == 3
    assert np.array_equal(h, S.finish(c))


def test_finish_stops_at_two_to_the_24(smk):
    c = np.zeros((256, 256), np.uint32)
    c[0, 0], c[9, 7], c[1, 1] = 2 ** 24 + 5, 1000, 2 ** 24
    h = _finish(smk, c)
    assert h[0, 0] == 255 and h[1, 1] == 255               # 2^24 + 5 finishes as 2^24
    assert h[9, 7] == int(np.float32(np.float32(np.log(1000.0)) / np.float32(np.log(float(2 ** 24))) * np.float32(255)))
    assert np.array_equal(h, S.finish(c))
    c[0, 0] = 2 ** 32 - 1
    assert np.array_equal(_finish(smk, c), h)


def test_finish_of_nothing_and_of_single_voxels_is_zero(smk):
    c = np.zeros((256, 256), np.uint32)
    assert not _finish(smk, c).any() and not S.finish(c).any()
    c[5, 5] = c[6, 6] = 1                                   # log 1 = 0: no bin holds more than one voxel
    assert not _finish(smk, c).any() and not S.finish(c).any()


def test_finish_on_random_counts(smk):
    rng = np.random.default_rng(5)
    c = (rng.integers(0, 5000, (256, 256)) * (rng.random((256, 256)) < 0.3)).astype(np.uint32)
    assert np.array_equal(_finish(smk, c), S.finish(c))
    data, _ = S.volume("u16", 2)
    assert np.array_equal(_finish(smk, S.counts(data)), S.finish(S.counts(data)))


def test_finish_refuses_null(smk):
    L = smk.load_library()
    c, h = np.zeros(65536, np.uint32), np.zeros(65536, np.uint8)
    assert L.smk_hist2d_finish(None, _p(h)) != 0
    assert L.smk_hist2d_finish(_p(c), None) != 0
    assert L.smk_hist2d_finish(_p(c), _p(h)) == 0
    with pytest.raises(ValueError):
        smk.Renderer.hist2d_finish(np.zeros(100, np.uint32))


# ---- u16 bins

def test_u16_bin_edges_and_the_integer_rule():
    for v, b in S.U16_EDGES:
        assert S.bin_u16(np.array([v]))[0] == b, v
    v = np.arange(65536, dtype=np.int64)
    assert np.array_equal(S.bin_u16(v), (255 * v) // 65535)     # floor(255 v / 65535), in integers
    assert S.bin_u16(np.array([65535], np.uint16))[0] == 255


# ---- the cases of the GPU tests

@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
def test_random_volumes_fill_many_bins(dtype):
    for seed in (1, 2):
        data, _ = S.volume(dtype, 2, seed)
        c = S.counts(data)
        assert np.count_nonzero(c) >= 2000 and int(c.sum()) == data.shape[0] * data.shape[1] * data.shape[2]
        assert c.max() >= 3 * 37 * 41                           # the uniform slices: whole waves in one bin


def test_whole_volume_is_more_than_one_flush_chunk():
    nx, ny, nz = S.DIMS
    assert nx * ny * nz > S.CHUNK and nx % 2 == ny % 2 == nz % 2 == 1


def test_shard_cases_reach_the_row_ends():
    """per voxel size (8-byte rows are evened out, 16-byte rows are not): some rank's region has an odd run length, some
    rank's rows start at an odd offset in the stored box, and every case has a rank with one of the two"""
    for u8 in (True, False):
        rows = {(n, h): [S.shard_rows(S.DIMS, r, n, h, u8) for r in range(n)] for n, h in S.SHARD_CASES}
        every = [rw for case in rows.values() for rw in case]
        assert any(nx & 1 for nx, _ in every) and any(ox & 1 for _, ox in every)
        for case, rw in rows.items():
            assert any(nx & 1 or ox & 1 for nx, ox in rw), case
    # the whole 8-byte volume: an odd run from offset 0 (the pad column behind it)
    assert S.shard_rows(S.DIMS, 0, 1, 1, True) == (41, 0)


def test_shard_regions_partition_the_volume():
    from simian_spacemonkey_amd import sortlast
    data, _ = S.volume("u8", 2)
    whole = S.counts(data)
    for n, _ in S.SHARD_CASES:
        parts = [S.counts(data, *sortlast.shard_region(S.DIMS, r, n)) for r in range(n)]
        assert np.array_equal(sum(p.astype(np.int64) for p in parts), whole)


def test_probe_restatement_on_a_hand_made_cell():
    data = np.arange(3 * 3 * 3 * 2, dtype=np.uint8).reshape(3, 3, 3, 2)
    raw, nrm, ok = S.probe(data, None, [(1, 0, 1), (2, 0, 0), (-1, 0, 0)])
    assert list(ok) == [True, False, False] and not raw[1:].any() and not nrm[1:].any()
    # corner i * 4 + j * 2 + k = voxel (x + k, y + j, z + i)
    assert raw[0, 0, 0] == data[1, 0, 1, 0] and raw[0, 1, 0] == data[1, 0, 2, 0] and raw[0, 2, 0] == data[1, 1, 1, 0]
    assert raw[0, 4, 1] == data[2, 0, 1, 1] and not raw[0, :, 2:].any() and (nrm[0] == 128).all()


# ---- the header

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smk.h")).read(), flags=re.S)


def test_new_entries_are_declared_bound_and_exported(smk):
    src = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in smk.ABI_SYMBOLS, name
        assert hasattr(smk.load_library(), name), name
    assert re.search(r"#define\s+SMK_STEP_CURRENT\s+\(-1\)", src) and smk.binding.STEP_CURRENT == -1
    for name in ("hist2d_step", "hist2d_step_device", "hist2d_finish", "probe_step"):
        assert callable(getattr(smk.Renderer, name)), name


def test_new_declarations_parse_as_c():
    """the header stays plain C: a C compiler accepts it and the five signatures it declares"""
    probe = "#include \"smk.h\"\n" \
            "int step_current[SMK_STEP_CURRENT == -1 ? 1 : -1];\n" \
            "int (*p0)(smk_ctx *, int, void *, void *) = smk_hist2d_step_device;\n" \
            "int (*p1)(smk_ctx *, int, unsigned *, unsigned char *) = smk_hist2d_step;\n" \
            "int (*p2)(const unsigned *, unsigned char *) = smk_hist2d_finish;\n" \
            "int (*p3)(smk_ctx *, int, const int *, int, float *, unsigned char *, int *) = smk_probe_step;\n"
    p = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=probe, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_driver_is_built():
    assert os.path.exists(os.path.join(ROOT, "tests", "host", "step_hist_main")), "build with __graft_entry__.build()"
