"""The library's one statement of the packed voxel and of a region's rows (csrc/smk_packed.h) without a GPU: its host side,
driven through tests/host/packed_main, against the restatements the tests own -- _step_read_ref.pack / unpack for the words,
Python's n // d for the exact division, _step_hist_ref.shard_rows / _layouts.stored_box and the closed form of the header's
comment for the rows -- and a walk over every unit of a region through the functions the kernels share: each voxel of the
region exactly once, none outside the stored box."""
import os
import subprocess

import numpy as np
import pytest

import _step_hist_ref as H
import _step_read_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "packed_main")


def ask(lines):
    """one answer line per question line"""
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    out = subprocess.run([EXE], input="".join(l + "\n" for l in lines), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines) and "bad line" not in out and "bad rows line" not in out
    return out


# ---- pack / unpack

U16_THIRD = [0, 1, 128, 255, 256, 257, 32767, 32768, 65534, 65535]
F32_BITS = [0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x80000000, 0x00000001, 0x807fffff, 0x00400000, 0x3f800000, 0]


def voxels(dtype, nelts):
    """(data [1][1][n][nelts], grad [1][1][n][3]): the shared random volume's first voxels, then the values that must not be
    missed -- in every channel, so in the u16 third channel and in .w of four-channel f32"""
    data, grad = R.volume(dtype, nelts)
    data, grad = data.reshape(-1, nelts)[:40], grad.reshape(-1, 3)[:40]
    if dtype == "u16":
        extra = np.array([[U16_THIRD[(i + 1) % 10], U16_THIRD[(i + 3) % 10], U16_THIRD[i]][:nelts] for i in range(10)], np.uint16)
    elif dtype == "u8":
        extra = np.array([[v] * nelts for v in (0, 1, 127, 128, 254, 255)], np.uint8)
    else:
        w = np.array([[F32_BITS[(i + e) % len(F32_BITS)] for e in range(nelts)] for i in range(len(F32_BITS))], np.uint32)
        extra = w.view(np.float32)
    g_extra = np.array([[0, 128, 255], [255, 0, 1]] * len(extra), np.uint8)[:len(extra)]
    data, grad = np.concatenate([data, extra]), np.concatenate([grad, g_extra])
    return np.ascontiguousarray(data).reshape(1, 1, -1, nelts), np.ascontiguousarray(grad).reshape(1, 1, -1, 3)


def hexes(line):
    return [int(x, 16) for x in line.split()]


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("dtype,nelts", R.LAYOUTS)
def test_pack_words_equal_the_restatement(dtype, nelts, with_normals):
    data, grad = voxels(dtype, nelts)
    if dtype == "u16" and nelts == 3:
        assert set(U16_THIRD) <= set(int(v) for v in data[..., 2].ravel())
    words, sep = R.pack(data, grad if with_normals else None)
    words, n = words.reshape(-1, words.shape[-1]), words.shape[2]
    g = grad.reshape(-1, 3).astype(int) if with_normals else np.full((n, 3), -1)
    if dtype == "f32":
        ch = np.zeros((n, 4), np.uint32)
        ch[:, :nelts] = R.bits(data).reshape(n, nelts)
        got = ask(["packf %d %d %d %d %08x %08x %08x %08x" % ((nelts,) + tuple(g[i]) + tuple(int(x) for x in ch[i])) for i in range(n)])
        for i, line in enumerate(got):
            assert hexes(" ".join(line.split()[:4])) == [int(x) for x in words[i]], (i, line)
            want_sep = "-" if sep is None else "%08x" % int(sep.reshape(-1)[i])
            assert line.split()[4] == want_sep, (i, line)
    else:
        ch = np.zeros((n, 4), np.int64)
        ch[:, :nelts] = data.reshape(n, nelts)
        got = ask(["pack8 %d %d %d %d %d %d %d %d %d" % ((R.CODE[dtype], nelts) + tuple(g[i]) + tuple(int(x) for x in ch[i])) for i in range(n)])
        for i, line in enumerate(got):
            assert hexes(line) == [int(x) for x in words[i]], (i, line)


@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("dtype,nelts", R.LAYOUTS)
def test_unpacked_words_equal_the_restatement(dtype, nelts, with_normals):
    """the restatement's words of the same voxels, and any 32 bits in every word: a decoder sees what a blend or a derive left"""
    data, grad = voxels(dtype, nelts)
    words, sep = R.pack(data, grad if with_normals else None)
    rng = np.random.default_rng(31 * R.CODE[dtype] + nelts)
    words = np.concatenate([words, rng.integers(0, 1 << 32, words.shape, dtype=np.uint64).astype(np.uint32)], 2)
    if sep is not None:
        sep = np.concatenate([sep, rng.integers(0, 1 << 32, sep.shape, dtype=np.uint64).astype(np.uint32)], 2)
    want_d, want_g = R.unpack(words, sep, dtype, nelts)
    w, n = words.reshape(-1, words.shape[-1]), words.shape[2]
    if dtype == "f32":
        s = ["-"] * n if sep is None else ["%08x" % int(x) for x in sep.reshape(-1)]
        got = ask(["unpackf %d %08x %08x %08x %08x %s" % ((nelts,) + tuple(int(x) for x in w[i]) + (s[i],)) for i in range(n)])
        rows = [[int(x, 16) for x in line.split()[:4]] + [int(x) for x in line.split()[4:]] for line in got]
    else:
        got = ask(["unpack8 %d %d %08x %08x" % (R.CODE[dtype], nelts, int(w[i][0]), int(w[i][1])) for i in range(n)])
        rows = [[int(x) for x in line.split()] for line in got]
    rows = np.array(rows, np.int64)
    assert np.array_equal(rows[:, :nelts], R.bits(want_d).reshape(n, nelts).astype(np.int64))
    assert not rows[:, nelts:4].any()                                     # (a channel the volume does not have)
    assert np.array_equal(rows[:, 4:], want_g.reshape(n, 3).astype(np.int64))


def test_q8_and_its_expansion_at_the_named_values():
    got = ask(["pack8 2 3 -1 0 0 0 0 %d 0" % v for v in U16_THIRD])
    q = [int(line.split()[1], 16) >> 24 for line in got]
    assert q == [int(x) for x in R.q8(U16_THIRD)] == [0, 0, 0, 1, 1, 1, 127, 128, 255, 255]
    back = ask(["unpack8 2 3 00000000 %02x808080" % x for x in q])
    assert [int(line.split()[2]) for line in back] == [257 * x for x in q]


# ---- the exact division

def test_division_is_exact():
    ds = {1, 2, 3, 5, 7, 2 ** 32 - 1}
    for k in range(1, 32):
        ds |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    pairs = []
    for d in sorted(ds):
        ns = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 ** 31, 2 ** 32 - 1}
        if d >= 2:
            ns.add(2 ** 32 - d)
        pairs += [(d, n) for n in sorted(ns) if 0 <= n < 2 ** 32]
    assert len(ds) >= 90 and len(pairs) > 700
    got = ask(["div %d %d" % p for p in pairs])
    wrong = [(d, n, int(g)) for (d, n), g in zip(pairs, got) if int(g) != n // d]
    assert wrong == []


# ---- the region's rows

def closed_form(g0, g1, o, wide):
    """(upr, head, tail, ox, units, nvox) as the header's comment states them"""
    nx, ny, nz, ox = g1[0] - g0[0], g1[1] - g0[1], g1[2] - g0[2], g0[0] - o[0]
    if wide:
        return nx, 0, 0, ox, nx * ny * nz, nx * ny * nz
    upr = (ox % 2 + nx + 1) // 2
    return upr, ox & 1, (ox + nx) & 1, ox // 2, upr * ny * nz, nx * ny * nz


@pytest.fixture(scope="module")
def row_cases(smk):
    """(dims, rank, nranks, halo, wide, g0, g1, O, D) of every region the walk covers"""
    from _layouts import stored_box
    from simian_spacemonkey_amd import sortlast
    cases = []
    for wide in (False, True):
        for dims in (R.SMALL, R.LONG, R.LONGER, H.DIMS):
            cases.append((dims, 0, 1, 1, wide))
        for nranks, halo in H.SHARD_CASES:
            cases += [(H.DIMS, rank, nranks, halo, wide) for rank in range(nranks)]
    out = []
    for dims, rank, nranks, halo, wide in cases:
        g0, g1 = sortlast.shard_region(dims, rank, nranks)
        o, d = stored_box(dims, rank, nranks, not wide, halo)
        out.append((dims, rank, nranks, halo, wide, tuple(g0), tuple(g1), tuple(o), tuple(d)))
    # plain integers, no context behind them: an even run between odd offsets (both ends masked), box and region off the origin
    for wide in (False, True):
        out.append(("plain", 0, 1, 0, wide, (5, 2, 2), (11, 5, 4), (2, 1, 1), (12, 6, 4)))
    return out


def test_rows_of_every_case_and_a_walk_over_their_units(row_cases):
    """chunks of 1024 units are the read-back's, 61440 (f32) and 30720 (8-byte) the histogram's, 7 is no divisor of anything"""
    cases = row_cases
    assert len(cases) == 2 * (5 + sum(n for n, _ in H.SHARD_CASES))
    asked = [(c, chunk) for c in cases for chunk in (1024, H.CHUNK if c[4] else H.CHUNK // 2, 7)]
    got = ask(["rows %d %d " % (c[4], chunk) + " ".join(str(v) for t in c[5:] for v in t) for c, chunk in asked])
    for ((dims, rank, nranks, halo, wide, g0, g1, o, d), chunk), line in zip(asked, got):
        what = (dims, rank, nranks, halo, wide, chunk)
        f = line.split()
        upr, head, tail, ox, units, nvox, outside = (int(x) for x in f[:7])
        assert (upr, head, tail, ox, units, nvox) == closed_form(g0, g1, o, wide), what
        if dims == H.DIMS:
            nx, off = H.shard_rows(dims, rank, nranks, halo, not wide)
            assert (nx, off) == (g1[0] - g0[0], g0[0] - o[0]), what
            assert (upr, head, tail, ox) == ((nx, 0, 0, off) if wide else ((off % 2 + nx + 1) // 2, off & 1, (off + nx) & 1, off // 2)), what
        assert outside == 0, what
        visits = np.frombuffer(f[7].encode(), np.uint8).astype(np.int64) - ord("0")
        assert visits.size == d[0] * d[1] * d[2], what
        want = np.zeros((d[2], d[1], d[0]), np.int64)
        want[g0[2] - o[2]:g1[2] - o[2], g0[1] - o[1]:g1[1] - o[1], g0[0] - o[0]:g1[0] - o[0]] = 1
        assert np.array_equal(visits.reshape(want.shape), want), what
        assert int(visits.sum()) == nvox


def test_the_cases_reach_masked_heads_and_tails_and_long_rows(row_cases):
    cases = [c for c in row_cases if not c[4]]
    forms = [closed_form(c[5], c[6], c[7], False) for c in cases]
    assert any(f[1] for f in forms) and any(f[2] for f in forms) and any(f[1] and f[2] for f in forms)
    assert any(f[0] > 1024 for f in forms) and any(not f[1] and not f[2] for f in forms)


@pytest.mark.parametrize("wide", [True, False])
def test_chunk_origin_and_lane_unit_of_regions_beyond_2_to_the_32_units(wide):
    """step_chunk_origin divides in 64 bits when the region has more than 2^32 - 1 units, by multiply-shift below that: both
    against Python's integers, at chunk starts on either side of 2^32 and at the region's ends"""
    big = ((3, 2, 1), (3003 if wide else 6004, 2002, 1001), (1, 0, 0), (3004 if wide else 6006, 2004, 1002))
    small = ((3, 2, 1), (303, 202, 101), (1, 0, 0), (306, 204, 102))
    asked = []
    for g0, g1, o, d in (big, small):
        upr, _, _, ox, units, _ = closed_form(g0, g1, o, wide)
        assert (units > 2 ** 32) == (g1 is big[1])
        bases = [0, upr - 1, upr, upr * (g1[1] - g0[1]) - 1, units // 2, units - 1]
        if units > 2 ** 32:
            bases += [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 32 + 61440 * 7]
        asked += [(g0, g1, o, d, b, i) for b in bases for i in (0, 1, 1023, 61439) if b + i < units]
    got = ask(["unit %d %d %d " % (wide, b, i) + " ".join(str(v) for t in (g0, g1, o, d) for v in t) for g0, g1, o, d, b, i in asked])
    for (g0, g1, o, d, b, i), line in zip(asked, got):
        upr, _, _, ox, _, _ = closed_form(g0, g1, o, wide)
        ny, pitch = g1[1] - g0[1], d[0] if wide else d[0] // 2
        row0, u0 = divmod(b, upr)
        z0, y0 = divmod(row0, ny)
        row, col = divmod(b + i, upr)
        z, y = divmod(row, ny)
        index = ((z + g0[2] - o[2]) * d[1] + y + g0[1] - o[1]) * pitch + ox + col
        assert [int(x) for x in line.split()] == [u0, y0, z0, row0, index, col, row - row0], (g0, g1, b, i)

