"""The column-stream kernel's plan rules (tests/_cols_plan_ref.py) swept without a GPU: what the kernel relies on holds for
every column size, voxel size, workgroup shape and knob setting, and every case of the GPU sweep
(tests/_cols_plan_cases.py) sits in the classes it was dialled to.

The sweep.  The ring's part of the plan sees a column only through its slice image's bytes, so every cw, ch in 1..255 is
reduced to the distinct slice sizes (checked against the voxel count for every pair), and those that fit LDS three times
run under both shapes and cols_ns 0 and 3..12.  The rules see a slice size only through its instruction count and the slots
that fit, so cols_fly 0..8 and cols_wstep 0..7 are crossed with all of that on one slice size per (n_ch, natural slots)."""
import numpy as np
import pytest

import _cols_plan_ref as ref
from _cols_plan_cases import BASES, CASES, CLASSES, REFUSED_CASE, TABLES_LDS, UNREACHABLE, classes_of, expected_plan

NS = [0] + list(range(3, 13))
FLY = list(range(9))
WSTEP = list(range(8))


def _slice_sizes(vb):
    """{slice bytes: a (cw, ch) that has them} over cw, ch in 1..255, each pair's bytes held to its voxel count"""
    n = np.arange(2, 257, dtype=np.int64)
    vox = n[:, None] * n[None, :]
    sb = (vox * vb + 15) // 16 * 16
    got = np.array([[ref.slice_bytes(cw, ch, vb) for ch in (1, 2, 7, 100, 255)] for cw in range(1, 256)])
    assert np.array_equal(got, sb[:, [0, 1, 6, 99, 254]])
    assert (sb % 16 == 0).all() and (sb >= vox * vb).all() and (sb - vox * vb < 16).all()
    out = {}
    for i, j in zip(*np.nonzero(sb <= (ref.LDS_CAP - ref.fixed_lds()) // 3)):
        out.setdefault(int(sb[i, j]), (int(n[i]) - 1, int(n[j]) - 1))
    return out


def _check(p, shape, ns, fly, wstep, tables):
    nl = ref.SHAPES[shape][1]
    assert 3 <= p["nslots"] <= 12 and (not ns or p["nslots"] <= ns)
    assert p["nslots"] * p["slice_bytes"] + ref.fixed_lds(tables) <= ref.LDS_CAP          # the ring beside the fixed part
    assert max(p["nslots"] * p["slice_bytes"], ref.MAX_RAYS * 16) + ref.fixed_lds(tables) <= ref.LDS_CAP   # ... or the set-up's scratch
    assert 1 <= p["last_units"] <= 64 and (p["n_ch"] - 1) * 1024 + p["last_units"] * 16 == p["slice_bytes"]
    assert p["n_ch"] <= 63
    assert p["n_ch"] * p["maxfly"] <= 63 or p["maxfly"] == 1
    assert p["n_ch"] * (p["maxfly"] - 1) <= 63                                             # the counted wait's immediate
    assert p["maxfly"] >= 1 and (p["maxfly"] * nl <= p["nslots"] - 2 or p["maxfly"] == 1)
    assert 0 <= p["wstep"] <= p["nslots"] - 2                                              # the load a consumer waits for is issued
    asked = wstep - 1 if wstep else None
    assert p["wstep"] == (min(asked, p["nslots"] - 2) if asked is not None else (0, 0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 2, 2)[p["nslots"]])
    if shape == 1:   # two loaders: the n_ch * maxfly <= 63 rule never binds (UNREACHABLE in tests/_cols_plan_cases.py)
        assert p["maxfly"] == max(1, min(fly or 2, (p["nslots"] - 2) // 2))


@pytest.mark.parametrize("vb", [8, 16])
def test_ring_rules_hold_for_every_slice_size_and_knob(vb):
    sizes = _slice_sizes(vb)
    assert len(sizes) > 1000
    full, seen, n = [], set(), 0
    for tables in (0, TABLES_LDS):
        for sb, (cw, ch) in sizes.items():
            try:
                nat = ref.ring(cw, ch, vb, tables=tables)
            except ref.Refused:
                assert 3 * sb + ref.fixed_lds(tables) > ref.LDS_CAP
                continue
            key = (nat["n_ch"], nat["nslots"], tables)
            if key not in seen:
                seen.add(key)
                full.append((cw, ch, tables))
            for shape in (0, 1):         # every slice size under every slot cap, the other knobs at their defaults
                for ns in NS:
                    _check(ref.ring(cw, ch, vb, shape=shape, ns=ns, tables=tables), shape, ns, 0, 0, tables)
                    n += 1
    for cw, ch, tables in full:          # one slice size per (n_ch, natural slots): every knob against every other
        for shape in (0, 1):
            for ns in NS:
                for fly in FLY:
                    for wstep in WSTEP:
                        _check(ref.ring(cw, ch, vb, shape=shape, ns=ns, fly=fly, wstep=wstep, tables=tables), shape, ns, fly, wstep, tables)
                        n += 1
    assert len(full) > 50 and n > 150000


def test_largest_slice():
    """31 instructions: the planner sizes columns for two slices in flight within the counted wait's 63"""
    p = ref.ring(43, 44, 16, ns=3, tables=TABLES_LDS)
    assert (p["n_ch"], p["last_units"], p["nslots"], p["maxfly"]) == (31, 60, 3, 1)
    with pytest.raises(ref.Refused, match="three times"):
        ref.ring(60, 60, 16)


def test_chunks_are_equal_and_entry_positions_fit_a_byte():
    for npos in list(range(1, 700)) + [1023, 1024, 1025, 2001, 2061, 4097, 65536]:
        for chunk in range(0, 300):
            cl, nck = ref.chunks(npos, chunk)
            most = 128 if chunk == 0 else min(max(chunk, 4), 256)
            assert 1 <= cl <= most and ref.entry_positions(npos, chunk) == cl - 1 < 256
            assert (nck - 1) * cl < npos <= nck * cl                      # nck chunks cover the positions, none is empty
            assert nck == ref.ceil_div(npos, most) or cl < most          # no more chunks than the limit needs
            # marching away from a pad slice it is position 0 of the first chunk, which must hold a real one too
            assert cl >= 2 or npos == 1
    assert ref.positions(41) == ref.positions(41, True, 1) == 40 and ref.positions(41, True, -1) == 41


def test_mask_words():
    for ncu, ncv, nck in ((1, 1, 1), (1, 1, 64), (1, 1, 65), (3, 2, 60), (3, 2, 61), (1, 1, 512), (2, 1, 511), (30, 20, 464)):
        nkeys, words = ref.keys(ncu, ncv, nck)
        assert nkeys == ncu + ncv + nck - 2 and 64 * (words - 1) < nkeys <= 64 * words <= 512
    for ncu, ncv, nck in ((1, 1, 513), (2, 2, 511), (255, 255, 5)):
        with pytest.raises(ref.Refused, match="more than 512 segment keys"):
            ref.keys(ncu, ncv, nck)


# ------------------------------------------------------------------------------------------------ the GPU sweep's cases
@pytest.mark.parametrize("c", [c for c in CASES if c["one"]], ids=lambda c: c["name"])
def test_case_sits_in_the_class_it_was_dialled_to(c):
    p = expected_plan(c)
    assert {k: p[k] for k in c["want"]} == c["want"], p
    assert set(c["cls"]) <= classes_of(c, p), (sorted(classes_of(c, p)), p)
    assert p["ncu"] == p["ncv"] == 1
    nx, ny, nz = c["dims"]
    assert nx * ny * nz * (16 if c["f32"] else 8) < 3 << 20 and max(c["size"]) <= 96


@pytest.mark.parametrize("c", [c for c in CASES if not c["one"]], ids=lambda c: c["name"])
def test_multi_column_case_whatever_its_columns(c):
    """the chunk and key classes of a case with several columns hold for every column size the planner may pick"""
    nx, ny, nz = c["dims"]
    assert nx * ny * nz * (16 if c["f32"] else 8) < 3 << 20 and max(c["size"]) <= 96
    if not c["want"]:
        return
    for cw in range(1, c["nu"]):
        for ch in range(1, c["nv"]):
            p = expected_plan(c, cw, ch)
            assert {k: p[k] for k in c["want"]} == c["want"], (cw, ch, p)
            assert {k for k in c["cls"] if k != "several columns"} <= classes_of(c, p)


def test_refused_case_is_refused_whatever_its_columns():
    c = REFUSED_CASE
    for cw in range(1, c["nu"]):
        for ch in range(1, c["nv"]):
            with pytest.raises(ref.Refused, match=c["refused"]):
                expected_plan(c, cw, ch)


def test_every_class_is_dialled_by_some_base():
    dialled = {k for b in BASES for k in b["cls"]}
    left = [k for k in CLASSES if k not in dialled and not k.startswith("ragged") and not k.endswith("cw != ch")]
    assert not left, left
    # the variants of a base cover both shapes (unless it pins one), both voxel types and the three axes
    by_base = {}
    for c in CASES:
        by_base.setdefault(c["base"], []).append(c)
    for b in BASES:
        v = by_base[b["name"]]
        assert {c["pose"][0] for c in v} == {"x", "y", "z"} and {c["f32"] for c in v} == {True, False}
        assert {c["shape"] for c in v} == ({b["shape"]} if b["shape"] else {1, 2})
        assert len({c["pose"][1] for c in v}) == 2
    assert UNREACHABLE == {("maxfly lowered by n_ch", "shape", 1)}
