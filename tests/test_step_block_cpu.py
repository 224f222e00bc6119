"""tests/_step_block_ref.py qualified (no GPU): over the ranks of every case the three cuts of the whole arrays cover what the
block entries can get wrong -- an odd x origin of a block, a rim that is not empty under cut (a), cells of the valid box that
straddle a region face, words that differ from the seeds on every rank with an interior voxel --, and C, the valid box and the
halo rule behave as smk.h says.  tests/test_gpu_step_block.py runs every case of the list."""
import numpy as np

import _step_block_ref as B
import _step_shard_ref as S


def all_cuts(ring="u8"):
    for case, (kind, dims, nranks, halo) in enumerate(B.CASES):
        for which in B.CUTS:
            for c in B.cuts_of(case, ring, which):
                yield case, kind, which, c


def test_every_block_lies_in_the_volume_and_its_c_contains_the_region(smk):
    for ring in B.RINGS:
        for case, kind, which, c in all_cuts(ring):
            for a in range(3):
                assert 0 <= c.origin[a] and c.size[a] > 0 and c.origin[a] + c.size[a] <= c.dims[a]
                assert c.O[a] <= c.lo[a] < c.hi[a] <= min(c.O[a] + c.D[a], c.dims[a])
            assert B.contains(c.lo, c.hi, c.g0, c.g1)
            assert B.contains(c.lo, c.hi, c.vlo, c.vhi) and B.contains(c.vlo, c.vhi, c.g0, c.g1)
            if which == "b":
                assert (c.lo, c.hi) == (c.stored_lo, c.stored_hi), "a view of the whole array: C is the stored box"
            else:
                assert (c.lo, c.hi) == (c.origin, tuple(o + s for o, s in zip(c.origin, c.size))), "the block lies inside the stored box"


def test_the_halo_rule(smk):
    seen_c = {k: 0 for k in B.REACH}
    for ring in B.RINGS:
        for case, kind, which, c in all_cuts(ring):
            halo = B.CASES[case][3]
            r = B.REACH[kind]
            if which == "c":                                # the block's halo, not the option's ...
                cut_inside = any((c.g0[a] > 0 and c.lo[a] > 0) or (c.g1[a] < c.dims[a] and c.hi[a] < c.dims[a]) for a in range(3))
                assert c.option_halo == halo + B.WIDER and c.src_halo == (r + 1 if cut_inside else c.option_halo) and c.halo == c.src_halo - r
                seen_c[kind] += cut_inside                  # (... unless the block reaches the volume's faces all round a thin volume)
            else:
                assert c.option_halo == halo == c.src_halo and c.halo == halo - r >= 1
            for a in range(3):                              # the result keeps its valid halo round the region, cut at the volume
                assert c.vlo[a] <= max(c.g0[a] - c.halo, 0) and c.vhi[a] >= min(c.g1[a] + c.halo, c.dims[a])
                assert c.vlo[a] == (0 if c.lo[a] == 0 else c.lo[a] + r) and c.vhi[a] == (c.dims[a] if c.hi[a] == c.dims[a] else c.hi[a] - r)
    assert all(n >= 20 for n in seen_c.values()), seen_c
    # an unsharded context: the block is the volume, nothing is lost
    c = B.Cut("derive", (7, 9, 11), 0, 1, 1, "u8", "a")
    assert (c.origin, c.size) == ((0, 0, 0), (7, 9, 11)) and (c.vlo, c.vhi) == ((0, 0, 0), (7, 9, 11)) and c.src_halo == c.halo == 1
    # a block one voxel short of the region on one side: C does not contain the region
    assert not B.contains(*B.c_box((75, 21, 19), (38, 0, 0), (37, 21, 19), (34, 0, 0), (42, 22, 19)), (37, 0, 0), (75, 21, 19))


def test_the_cases_cover_the_ground(smk):
    odd = {k: False for k in B.REACH}
    for case, kind, which, c in all_cuts("u8"):
        odd[kind] |= c.origin[0] % 2 == 1 and c.origin[0] != c.O[0]
    assert all(odd.values()), "an odd x origin of a block that is not the stored box's (the output's units stay even there)"
    for ring in B.RINGS:
        rim_a = {k: 0 for k in B.REACH}
        rims = {}
        for case, kind, which, c in all_cuts(ring):
            rims[case] = rims.get(case, False) or bool(c.rim().any())
            if which == "a":
                # (a) is narrower than the stored box wherever the row evening took a voxel: a rim beyond the reach's
                wider = (c.lo, c.hi) != (c.stored_lo, c.stored_hi)
                assert wider == (ring != "f32" and any((c.hi[a] - c.lo[a]) != c.stored_hi[a] - c.stored_lo[a] for a in range(3)))
                rim_a[kind] += wider
            cells = S.cells_of(c.vlo, c.vhi)
            assert S.straddles(cells, c.g0, c.g1).any(), "cells of the valid box that straddle a region face"
        # (every rank of a volume 3 voxels thick stores all of it: nothing is cut, no rim)
        assert len(rims) == len(B.CASES) and all(rims[i] == (B.CASES[i][1][0] > 3) for i in rims), "a rank whose result has a rim, per case"
        if ring != "f32":
            assert all(rim_a.values()), rim_a
    # the packed form (reach 0): under cut (a) the rim is what the evening added, and it exists for 8-byte voxels
    assert any(c.rim().any() for case in range(len(B.CASES)) for c in B.cuts_of(case, "u8", "a", reach=0))
    assert not any(c.rim().any() for case in range(len(B.CASES)) for c in B.cuts_of(case, "u8", "b", reach=0))


def test_every_rank_with_an_interior_voxel_moves_the_words(smk):
    hit = {k: [0, 0] for k in B.REACH}
    for case, (kind, dims, nranks, halo) in enumerate(B.CASES):
        for ring in B.RINGS:
            F = B.M.fields(ring, 2, dims)
            for c in B.cuts_of(case, ring, "a"):
                inner = S.has_interior(dims, c.g0, c.g1)
                w = B.region_words(kind, F, c.g0, c.g1)
                assert np.array_equal(w, B.SEEDS[kind]) == (not inner), (kind, dims, ring, c.rank, w)
                if inner and kind == "derive":               # both V words moved, and they bracket a real range
                    vmin, vmax = S.derive_extremes(w)[:2]
                    assert np.isfinite([vmin, vmax]).all() and vmin < vmax
                hit[kind][int(inner)] += 1
    assert all(a and b for a, b in hit.values()), "ranks with and without an interior voxel: %s" % hit


def test_take_cuts_the_whole_array(smk):
    dims = (75, 21, 19)
    whole = np.arange(np.prod(dims), dtype=np.float32).reshape(dims[::-1])
    for which in B.CUTS:
        for c in B.cuts_of(0, "u8", which):
            a, off, py, pz = c.take(whole, B.POISON["f32"])
            py, pz = py or c.size[0], pz or c.size[0] * c.size[1]
            flat = a.reshape(-1)
            (ox, oy, oz), (sx, sy, sz) = c.origin, c.size
            for z, y, x in ((0, 0, 0), (sz - 1, sy - 1, sx - 1), (sz // 2, sy // 3, sx // 2)):
                assert flat[off + z * pz + y * py + x] == whole[oz + z, oy + y, ox + x]
            if c.view:
                assert (flat == B.POISON["f32"]).sum() == whole.size - sx * sy * sz
