"""tests/_step_merge_h_shard_ref.py qualified (no GPU): from the NumPy restatement alone, the GPU tests of
tests/test_gpu_step_merge_h_shard.py cannot pass vacuously -- every rank's valid box holds more than its region, some rank has
a rim, the extremes are spread over the ranks, and a stencil of reach 1 would be wrong where one of reach 2 is exact."""
import numpy as np
import pytest

import _step_merge_h_ref as H
import _step_merge_h_shard_ref as R
import _step_shard_ref as S


def boxes(dims, nranks, halo, ring):
    return [R.stored_box(dims, r, nranks, halo, ring) for r in range(nranks)]


def test_the_cases_and_layouts_are_the_issues(smk):
    assert [c[0] for c in R.CASES] == [(75, 21, 19), (74, 21, 19), (75, 21, 19), (7, 9, 11), (3, 21, 19)]
    assert [c[1:] for c in R.CASES] == [(2, 3), (4, 4), (8, 3), (2, 3), (2, 3)]
    assert all(h >= R.REACH + 1 for _, _, h in R.CASES)
    for ring in R.RINGS:
        first = R.layouts(0, ring)
        assert {f[1:] for f in first} == set(H.FLAGS), "every (add_h, blur, compat) on the first case"
        assert {f[0] for f in first if f[1]} == set(H.NFS[ring]) and R.BLUR_ONLY[ring] in {f[0] for f in first if not f[1]}
        for case in range(1, len(R.CASES)):
            ls = R.layouts(case, ring)
            assert {f[1:] for f in ls} == {(1, 1, 1), (0, 1, 1)}
            assert {f[0] for f in ls if f[1]} == set(H.NFS[ring]) and {f[0] for f in ls if not f[1]} == {R.BLUR_ONLY[ring]}
        for case in range(len(R.CASES)):
            for nf, add_h, blur, compat in R.layouts(case, ring):
                assert 2 <= nf + 1 + add_h <= (3 if ring == "u16" else 4) and (not add_h or ring != "u16" or nf == 1)
    # the tile's edges: a stored box wider than a tile and thicker than 8 in y and z; both parities of a rank's x origin; a pad
    # column on one rank and not on another; a rank whose region is border alone
    bx = boxes((75, 21, 19), 2, 3, "u8")
    assert any(D[0] > R.TILE[0] and D[1] > R.TILE[1] and D[2] > R.TILE[2] for _, _, _, D, _ in bx) and bx[1][2][0] % 2 == 1
    assert R.stored_box((74, 21, 19), 1, 4, 4, "u8")[2][0] % 2 == 0
    assert [b[4][0] for b in boxes((7, 9, 11), 2, 3, "u8")] == [False, True]
    inner = [S.has_interior((3, 21, 19), b[0], b[1]) for b in boxes((3, 21, 19), 2, 3, "u8")]
    assert inner == [False, True]


@pytest.mark.parametrize("ring", R.RINGS)
def test_every_valid_box_holds_a_halo_voxel_and_some_rank_has_a_rim(smk, ring):
    for dims, nranks, halo in R.CASES:
        rim = False
        for g0, g1, O, D, pad in boxes(dims, nranks, halo, ring):
            lo, hi = R.valid_box(dims, O, D, R.REACH)
            slo, shi = S.uploaded_valid(dims, O, D)
            assert all(lo[a] <= g0[a] and g1[a] <= hi[a] for a in range(3)), "the valid box contains the region"
            assert any(lo[a] < g0[a] or g1[a] < hi[a] for a in range(3)), "... and a halo voxel"
            for a in range(3):                              # one voxel at least beyond every face of the region that is cut
                assert g0[a] == 0 or lo[a] <= g0[a] - 1
                assert g1[a] == dims[a] or hi[a] >= g1[a] + 1
            rim |= (lo, hi) != (slo, shi)
            assert all(slo[a] <= lo[a] and hi[a] <= shi[a] for a in range(3))
        # (the 3-voxel-thick volume: halo 3 makes every rank store all of it, so no box is cut and there is no rim to have)
        cut = any(S.cut_anywhere(dims, b[2], b[3]) for b in boxes(dims, nranks, halo, ring))
        assert cut == (dims[0] != 3) and rim == cut, (dims, nranks)


def ranks_words(case, ring, nf, add_h, compat):
    dims, nranks, halo = R.CASES[case]
    F = R.fields(case, ring, nf)
    return F, [R.region_words(F, *R.stored_box(dims, r, nranks, halo, ring)[:2], add_h, compat) for r in range(nranks)]


@pytest.mark.parametrize("ring", R.RINGS)
def test_the_extremes_are_spread_over_the_ranks(smk, ring):
    """the words of the whole volume as one region are the maximum of the ranks' words in every case; in the first three cases
    the three extremes are not all rank 0's, and every rank's words differ from the combined words"""
    for case, (dims, nranks, halo) in enumerate(R.CASES):
        for nf in H.NFS[ring]:
            for compat in (0, 1):
                F, words = ranks_words(case, ring, nf, 1, compat)
                whole = R.region_words(F, (0, 0, 0), dims, 1, compat)
                both = R.combine(words)
                assert np.array_equal(both, whole), (case, nf, compat)
                assert (whole[3:] == R.INT_MIN).all() and not np.array_equal(whole[:3], R.WORD_SEEDS[:3])
                assert whole[1] != R.WORD_SEEDS[1] and whole[2] != R.WORD_SEEDS[2], "H has extremes"
                if case < 3:
                    assert not np.array_equal(words[0][:3], both[:3]), (case, nf, compat, "all three extremes lie in rank 0's region")
                    for r, w in enumerate(words):
                        assert not np.array_equal(w[:3], both[:3]), (case, nf, compat, r)
        # without H the H words keep their seeds
        F, words = ranks_words(case, ring, H.NFS[ring][-1], 0, 1)
        assert all(np.array_equal(w[1:], R.WORD_SEEDS[1:]) for w in words) and R.combine(words)[0] > 0
    # a region without an interior voxel exports the seeds
    F, words = ranks_words(4, ring, 1, 1, 1)
    assert np.array_equal(words[0], R.WORD_SEEDS) and not np.array_equal(words[1], R.WORD_SEEDS)


def test_the_restatements_extremes_are_the_one_call_restatements(smk):
    """region_words over the whole volume against _step_merge_h_ref's own extremes (h_extremes applies the +-1e8 seeds, which
    no extreme of these fields reaches)"""
    for ring in R.RINGS:
        F = R.fields(0, ring, 1)
        w = R.region_words(F, (0, 0, 0), R.CASES[0][0], 1, 1)
        mag, hs, _, _ = R.unscaled(F, 1)
        hmin, hmax = H.h_extremes(hs, ring != "u8")
        mx, lo, hi = R.words_extremes(w)
        assert np.float32(lo) == hmin and np.float32(hi) == hmax and mx == float(mag[1:-1, 1:-1, 1:-1].max())


def test_complement_and_ordering_round_trip():
    vals = np.array([-np.inf, -1e8, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, 1e8, np.inf], np.float32)
    o = R.ordered(vals).astype(np.int64)
    assert (np.diff(o) > 0).all(), "ascending with the float, -0 below +0"
    assert np.array_equal(S.unordered(o.astype(np.int32)).view(np.uint32), vals.view(np.uint32))
    c = ~o.astype(np.int32)
    assert (np.diff(c.astype(np.int64)) < 0).all(), "a complement descends: the maximum of complements is the minimum"
    assert np.array_equal(~c, o.astype(np.int32))
    assert int(~c.max()) == int(o.min()) and float(S.unordered(~c.max())) == -np.inf
    # the seeds: nothing is below them, they round-trip, and a maximum over seeds alone leaves them
    assert R.WORD_SEEDS[0] == int(R.ordered(0.0)) and ~R.WORD_SEEDS[1] == int(R.ordered(np.inf)) and R.WORD_SEEDS[2] == int(R.ordered(-np.inf))
    assert R.words_extremes(R.WORD_SEEDS) == (0.0, np.inf, -np.inf)
    assert np.array_equal(R.combine([R.WORD_SEEDS, R.WORD_SEEDS]), R.WORD_SEEDS)
    fin = np.array([-3.0, 7.5], np.float32)
    w = R.WORD_SEEDS.copy()
    w[1], w[2] = ~int(R.ordered(fin).min()), int(R.ordered(fin).max())
    assert np.array_equal(R.combine([R.WORD_SEEDS, w]), w) and R.words_extremes(w)[1:] == (-3.0, 7.5)
    assert (R.WORD_SEEDS[3:] == R.INT_MIN).all()


@pytest.mark.parametrize("ring", R.RINGS)
def test_the_reach_is_two_and_not_one(smk, ring):
    """H and the blurred normal recomputed with zeros beyond a rank's stored box: at distance 1 from a cut face some voxel
    differs from the exact value, from distance 2 on every voxel is exact -- and that is the valid box"""
    case = 0
    dims, nranks, halo = R.CASES[case]
    F = R.fields(case, ring, 1)
    _, hs, nb, _ = R.unscaled(F, 1)
    for r in range(nranks):
        g0, g1, O, D, pad = R.stored_box(dims, r, nranks, halo, ring)
        lo, hi = S.uploaded_valid(dims, O, D)
        _, hz, nz_, _ = R.unscaled(R.zeroed_outside(F, lo, hi), 1)
        d = R.cut_distance(dims, lo, hi)
        interior = np.zeros(d.shape, bool)
        interior[1:-1, 1:-1, 1:-1] = True
        ok_h = R.same_bits(hs, hz)
        ok_n = R.same_bits(nb, nz_).all(-1)
        at1 = (d == 1) & interior
        assert at1.any() and (~ok_h[at1]).any(), "rank %d: H at distance 1 from a cut face reads a voxel the box does not hold" % r
        assert (~ok_n[at1]).any(), "rank %d: so does the blurred normal" % r
        far = d >= 2
        assert far.any() and ok_h[far].all() and ok_n[far].all(), "rank %d: exact from distance 2 on" % r
        vlo, vhi = R.valid_box(dims, O, D, R.REACH)
        assert np.array_equal(far, R.in_box(d.shape, (0, 0, 0), vlo, vhi)), "distance >= 2 is the valid box"
        # a reach of 1 would have been enough for the plain gradient alone, which smk_merge_timestep_shard serves
        _, _, _, plain = R.unscaled(F, 1)
        _, _, _, plain_z = R.unscaled(R.zeroed_outside(F, lo, hi), 1)
        assert R.same_bits(plain, plain_z).all(-1)[d >= 1].all()
