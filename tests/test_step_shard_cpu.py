"""tests/_step_shard_ref.py qualified (no GPU): its case list covers what the stencil producers on a shard can get wrong, its
stored box is the one sortlast.py's shard rule and the upload's evening rule give, its valid boxes and words behave as
smk.h says.  tests/test_gpu_step_shard.py runs every case of the list."""
import numpy as np

import _step_shard_ref as S


def boxes(kind, dims, nranks, halo, ring):
    return [S.stored_box(dims, r, nranks, halo, ring) for r in range(nranks)]


def test_the_cases_cover_the_ground(smk):
    ranks = {k: set() for k in S.REACH}
    halos = {k: set() for k in S.REACH}
    for kind, dims, nranks, halo in S.CASES:
        ranks[kind].add(nranks)
        halos[kind].add(halo)
        assert halo >= S.REACH[kind] + 1, "the source's valid halo must be reach + 1"
    assert ranks["derive"] >= {2, 4, 8} and ranks["merge"] >= {2, 4, 8}
    assert halos["derive"] >= {3, 4} and halos["merge"] >= {2, 3}
    assert any(all(n % 2 for n in dims) for _, dims, _, _ in S.CASES), "an all-odd volume"
    # both parities of a rank's x origin, for 8-byte voxels
    par = set()
    for kind, dims, nranks, halo in S.CASES:
        for g0, g1, O, D, pad in boxes(kind, dims, nranks, halo, "u8"):
            assert D[0] % 2 == 0 and D[1] % 2 == 0
            if O[0] > 0:
                par.add((kind, O[0] % 2))
    assert par >= {("derive", 0), ("derive", 1), ("merge", 0), ("merge", 1)}, par
    assert S.stored_box((75, 21, 19), 1, 2, 3, "u8")[2][0] % 2 == 1 and S.stored_box((74, 21, 19), 1, 4, 4, "u8")[2][0] % 2 == 0
    # a stored box wider than the derive's tile and thicker than 8 voxels in y and z
    assert any(kind == "derive" and D[0] > S.DERIVE_TILE[0] and D[1] > 8 and D[2] > 8
               for kind, dims, nranks, halo in S.CASES for _, _, _, D, _ in boxes(kind, dims, nranks, halo, "u8"))
    # ... and wider than one tile row of the merge kernels, for each ring
    for ring in S.RINGS:
        assert any(kind == "merge" and D[0] > S.MERGE_TILE_X[ring]
                   for kind, dims, nranks, halo in S.CASES for _, _, _, D, _ in boxes(kind, dims, nranks, halo, ring)), ring
    # a volume 3 voxels thick along a split axis: one rank's region has no interior voxel, another's has
    for want in S.REACH:
        hit = False
        for kind, dims, nranks, halo in S.CASES:
            if kind != want or dims[0] != 3:
                continue
            inner = [S.has_interior(dims, b[0], b[1]) for b in boxes(kind, dims, nranks, halo, "u8")]
            hit |= (not all(inner)) and any(inner)
        assert hit, want
    # the pad column on one rank and not on another
    assert any(len({b[4][0] for b in boxes(kind, dims, nranks, halo, "u8")}) == 2 for kind, dims, nranks, halo in S.CASES)
    assert [b[4][0] for b in boxes("derive", (7, 9, 11), 2, 3, "u8")] == [False, True]


def test_the_stored_box_holds_the_region_and_its_halo(smk):
    for kind, dims, nranks, halo in S.CASES:
        for ring in S.RINGS:
            seen = np.zeros(dims[::-1], np.int32)
            for g0, g1, O, D, pad in boxes(kind, dims, nranks, halo, ring):
                seen[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]] += 1
                for a in range(3):
                    assert O[a] <= max(g0[a] - halo, 0) and min(g1[a] + halo, dims[a]) <= O[a] + D[a] <= dims[a] + pad[a]
                    assert max(g0[a] - halo, 0) - O[a] <= 1, "the evening rule adds one voxel at the most"
                    assert not pad[a] or (ring != "f32" and a < 2 and O[a] == 0 and O[a] + D[a] == dims[a] + 1)
            assert (seen == 1).all()


def test_the_valid_box_keeps_a_halo_voxel_and_the_rim_is_what_is_left(smk):
    for kind, dims, nranks, halo in S.CASES:
        r = S.REACH[kind]
        for ring in S.RINGS:
            for g0, g1, O, D, pad in boxes(kind, dims, nranks, halo, ring):
                lo, hi = S.valid_box(dims, O, D, r)
                for a in range(3):
                    # the region and halo - reach >= 1 voxels round it, cut at the volume
                    assert lo[a] <= max(g0[a] - (halo - r), 0) and hi[a] >= min(g1[a] + (halo - r), dims[a])
                    assert (lo[a] == 0) == (O[a] == 0) or O[a] > 0
                    assert lo[a] == (0 if O[a] == 0 else O[a] + r)
                    assert hi[a] == (dims[a] if O[a] + D[a] >= dims[a] else O[a] + D[a] - r)
                inside = S.in_box(D[::-1], O, lo, hi)
                vol = S.in_box(D[::-1], O, (0, 0, 0), dims)
                rim = vol & ~inside
                assert inside.any() and not (inside & ~vol).any()
                assert rim.any() == S.cut_anywhere(dims, O, D)
                assert S.valid_halo_after(nranks, halo, r) == halo - r >= 1
                # a second stencil shrinks from the first one's valid box
                lo2, hi2 = S.valid_box(dims, O, D, r, (lo, hi))
                for a in range(3):
                    assert lo2[a] == (0 if O[a] == 0 else O[a] + 2 * r) and hi2[a] == (dims[a] if O[a] + D[a] >= dims[a] else O[a] + D[a] - 2 * r)
    # an unsharded context: no rim, the valid halo stays
    g0, g1, O, D, pad = S.stored_box((7, 9, 11), 0, 1, 1, "u8")
    assert O == (0, 0, 0) and D == (8, 10, 11) and pad == (True, True, False)
    assert S.valid_box((7, 9, 11), O, D, 2) == ((0, 0, 0), (7, 9, 11)) and S.valid_halo_after(1, 1, 2) == 1


def test_probe_cells_and_straddling(smk):
    g0, g1, O, D, pad = S.stored_box((75, 21, 19), 1, 2, 3, "u8")
    lo, hi = S.valid_box((75, 21, 19), O, D, 2)
    cells = S.cells_of(lo, hi)
    assert len(cells) == np.prod([hi[a] - lo[a] - 1 for a in range(3)])
    st = S.straddles(cells, g0, g1)
    assert st.any() and not st.all()
    assert (cells[st][:, 0] == g0[0] - 1).all(), "x is the only split axis: the straddling cells sit on the region's low x face"


def test_the_words_combine_by_maximum():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(0, 1e3, 64), [-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e38, -3e38]]).astype(np.float32)
    o = S.ordered(x)
    order = np.argsort(x, kind="stable")             # (-0.0 stands before 0.0 in x, and its ordered int is the smaller)
    assert (np.diff(o[order].astype(np.int64)) >= 0).all(), "the ordered int ascends with the float"
    assert np.array_equal(S.unordered(o).view(np.uint32), x.view(np.uint32))
    # minima travel complemented: the maximum of the complements is the complement of the minimum
    parts = [x[i::4] for i in range(4)]
    words = [S.derive_words(p.min(), p.max(), p.min() * 2, p.max() * 2, p.min() - 1, p.max() + 1) for p in parts]
    got = S.combine(words)
    want = S.derive_words(x.min(), x.max(), x.min() * 2, x.max() * 2, x.min() - 1, x.max() + 1)
    assert np.array_equal(got, want) and (got[6:] == S.INT_MIN).all()
    assert S.derive_extremes(got)[:2] == (float(x.min()), float(x.max()))
    # the seeds are neutral, and are what a rank without an interior voxel sends
    assert np.array_equal(S.combine([S.DERIVE_SEEDS, words[0]]), words[0])
    assert S.derive_extremes(S.DERIVE_SEEDS) == (np.inf, -np.inf) * 3
    m = [S.merge_words(v) for v in (0.0, 17.5, 3.0)]
    assert np.array_equal(S.combine(m), S.merge_words(17.5)) and np.array_equal(S.combine([S.MERGE_SEEDS, m[2]]), m[2])
    assert S.MERGE_SEEDS[0] == int(S.ordered(0.0)) == 0


def test_sources_and_placement(smk):
    for kind, nelts in (("derive", 3), ("merge", 3)):
        for ring in S.RINGS:
            d, n = S.source(kind, ring, (7, 9, 11))
            assert d.shape == (11, 9, 7, nelts) and n.shape == (11, 9, 7, 3) and d.dtype == S.M.NP[ring]
    d, _ = S.source("merge", "f32", (7, 9, 11), nf=3)
    assert d.shape[-1] == 4
    dims = (75, 21, 19)
    vol = np.arange(np.prod(dims), dtype=np.float32).reshape(dims[::-1] + (1,))
    parts = []
    for r in range(8):
        g0, g1, _, _, _ = S.stored_box(dims, r, 8, 3, "f32")
        parts.append((g0, vol[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]]))
    assert np.array_equal(S.place(dims, 1, np.float32, parts), vol)
