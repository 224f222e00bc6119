"""Reading a resident time step back, without a GPU: the NumPy restatement of the pack and of the download rule
(tests/_step_read_ref.py) proved on itself -- unpack o pack is the identity for u8 and f32 bits, a u16 third channel comes
back as 257 * q8(c) and packs to the same voxel again, the shard regions tile the volume exactly once -- which qualifies the
cases tests/test_gpu_step_read.py runs; and the three new declarations of the header, bound and exported."""
import os
import re
import subprocess

import numpy as np
import pytest

import _step_read_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["smk_get_timestep_box", "smk_download_timestep_device", "smk_download_timestep"]


# ---- the restatement

@pytest.mark.parametrize("dtype, nelts", D.LAYOUTS)
@pytest.mark.parametrize("normals", [True, False])
def test_unpack_of_pack(dtype, nelts, normals):
    data, grad = D.volume(dtype, nelts)
    grad = grad if normals else None
    words, sep = D.pack(data, grad)
    assert words.shape[-1] == (4 if dtype == "f32" else 2)
    assert (sep is not None) == (dtype == "f32" and nelts == 4 and normals)
    got, gn = D.unpack(words, sep, dtype, nelts)
    want, wn = D.expected(data, grad)
    assert got.dtype == data.dtype and np.array_equal(D.bits(got), D.bits(want))
    assert np.array_equal(gn, wn) and (normals or (gn == 128).all())
    if dtype != "u16" or nelts < 3:                         # the identity, bit for bit
        assert np.array_equal(D.bits(got), D.bits(data))
    else:
        assert np.array_equal(got[..., :2], data[..., :2]) and not np.array_equal(got[..., 2], data[..., 2])
    # what comes back packs to the same voxels: upload(download(step)) stores the step again
    again, sep2 = D.pack(got, gn if normals else None)
    assert np.array_equal(again, words) and (sep is None or np.array_equal(sep, sep2))


def test_f32_volumes_hold_the_patterns_a_float_copy_could_lose():
    w = D.volume("f32", 4)[0].view(np.uint32)
    f = w.view(np.float32)
    assert np.isnan(f).any() and np.isinf(f).any()
    nan = w[np.isnan(f)]
    assert len(np.unique(nan & 0x7fffff)) > 4               # NaN payloads
    assert ((nan & 0x400000) == 0).any()                    # ... signalling ones among them
    assert (w == 0x80000000).any()                          # -0
    assert (((w & 0x7f800000) == 0) & ((w & 0x7fffff) != 0)).any()     # denormals


def test_every_u16_third_channel_value():
    c = np.arange(65536, dtype=np.uint16).reshape(16, 64, 64, 1)
    data = np.concatenate([c, c[::-1], c], -1)
    words, _ = D.pack(data)
    got, _ = D.unpack(words, None, "u16", 3)
    q = D.q8(np.arange(65536))
    assert q.min() == 0 and q.max() == 255 and np.array_equal(np.unique(q), np.arange(256))
    assert np.array_equal(got[..., 2].ravel(), 257 * q)
    assert np.array_equal(D.q8(got[..., 2].ravel()), q)     # idempotence: q8(257 q) == q
    assert np.array_equal(D.q8(257 * np.arange(256)), np.arange(256))
    assert np.array_equal(got[..., :2], data[..., :2])


@pytest.mark.parametrize("dims", [(41, 37, 45), D.SMALL, (2, 2, 2), (10, 3, 7)])
def test_shard_regions_tile_the_volume_once(smk, dims):
    from simian_spacemonkey_amd import sortlast           # (importable once the smk fixture has loaded the package)
    rng = np.random.default_rng(3)
    vol = rng.integers(0, 256, dims[::-1] + (2,), dtype=np.uint8)
    for nranks in (1, 2, 4, 8):
        seen = np.zeros(dims[::-1], np.int32)
        whole = np.zeros_like(vol)
        for rank in range(nranks):
            g0, g1 = D.region(dims, rank, nranks)
            assert (g0, g1) == tuple(map(tuple, sortlast.shard_region(dims, rank, nranks)))
            seen[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]] += 1
            whole[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]] = D.cut(vol, g0, g1)
        assert (seen == 1).all() and np.array_equal(whole, vol), (dims, nranks)


def test_the_small_volume_reaches_every_byte_phase():
    """9 x 3 bytes per row: the rows of a three-byte output start on every phase of a dword"""
    nx = D.SMALL[0]
    assert all(n % 2 for n in D.SMALL) and {(r * nx * 3) % 4 for r in range(8)} == {0, 1, 2, 3}
    # a row of more 16-byte units than the 1024 one workgroup takes at a time: 1100 f32 voxels; 2101 8-byte voxels are 1051
    assert D.LONG[0] > 1024 and (D.LONGER[0] + 1) // 2 > 1024 and D.LONGER[0] % 2 == 1 and (D.LONGER[0] * 3) % 4 != 0


# ---- the header, the binding, the driver

def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smk.h")).read(), flags=re.S)


def test_new_entries_are_declared_bound_and_exported(smk):
    src = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in smk.ABI_SYMBOLS, name
        assert hasattr(smk.load_library(), name), name
    for name in ("timestep_box", "download_timestep_device", "download_timestep"):
        assert callable(getattr(smk.Renderer, name)), name


def test_the_library_exports_nothing_else_new(smk):
    out = subprocess.run(["nm", "-D", "--defined-only", smk.library_path()], capture_output=True, text=True).stdout
    mine = {ln.split()[-1] for ln in out.splitlines() if re.search(r"\s[TW]\s+smk_\w+$", ln)}
    assert set(NEW) <= mine and mine <= set(smk.ABI_SYMBOLS), sorted(mine - set(smk.ABI_SYMBOLS))


def test_new_declarations_parse_as_c():
    probe = "#include \"smk.h\"\n" \
            "int (*p0)(smk_ctx *, int *, int *, int *, smk_dtype *, int *) = smk_get_timestep_box;\n" \
            "int (*p1)(smk_ctx *, int, void *, void *, void *) = smk_download_timestep_device;\n" \
            "int (*p2)(smk_ctx *, int, void *, unsigned char *) = smk_download_timestep;\n"
    p = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=probe, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_the_header_sends_a_blends_derivatives_to_the_download():
    src = open(os.path.join(ROOT, "include", "smk.h")).read()
    at = src.index("not derivatives of the blended scalar")
    assert "smk_download_timestep_device" in src[at:at + 400]


def test_driver_is_built():
    assert os.path.exists(os.path.join(ROOT, "tests", "host", "step_download_main")), "build with __graft_entry__.build()"
