"""tests/_step_chain_ref.py qualified (no GPU): the mask model of what is valid after a chain of producers agrees with the
box rules the suite already trusts on every single link, every step of every chain case stays a box, every case has a rank
with a telling face -- a side where the stored box ends on the volume's face while the stencil's source does not --, no link
lacks its valid halo, and the case list covers the rings, an odd x origin and a stored box wider than a derive tile.
tests/test_gpu_step_chain.py runs every case of the list."""
import numpy as np
import pytest

import _step_block_ref as B
import _step_chain_ref as C
import _step_shard_ref as S


def every_rank():
    for case, (cid, dims, nranks, halo, links) in enumerate(C.CASES):
        for ring in C.RINGS:
            for R in C.ranks_of(case, ring):
                yield cid, ring, R, links, C.run(R, links)


def test_erosion_and_boxes():
    m = C.box_mask((7, 5, 4), (2, 0, 1), (7, 4, 4))
    assert m.sum() == 5 * 4 * 3 and C.box_of(m) == ((2, 0, 1), (7, 4, 4))
    # faces of the volume lose nothing, the others lose r
    assert C.box_of(C.erode(m, 1)) == ((3, 0, 2), (7, 3, 4))
    assert C.box_of(C.erode(m, 2)) == ((4, 0, 3), (7, 2, 4))
    assert C.box_of(C.erode(np.ones((4, 5, 7), bool), 2)) == ((0, 0, 0), (7, 5, 4))
    assert C.box_of(np.zeros((4, 5, 7), bool)) is None
    two = m.copy()
    two[0, 0, 0] = True
    assert C.box_of(two) is None, "two boxes are no box"
    # one invalid voxel takes its whole neighbourhood
    hole = np.ones((9, 9, 9), bool)
    hole[4, 4, 4] = False
    assert (~C.erode(hole, 2)).sum() == 125 and (~C.erode(hole, 1)).sum() == 27
    # two erosions of r are one of 2 r
    assert np.array_equal(C.erode(C.erode(m, 1), 1), C.erode(m, 2))


def test_the_mask_stays_a_box():
    n = 0
    for cid, ring, R, links, steps in every_rank():
        for out, st in steps.items():
            assert st.box is not None, (cid, ring, R.rank, out)
            lo, hi = st.box
            # inside the stored box and the volume, and round the region with the step's valid halo, cut at the volume
            assert all(R.stored_lo[a] <= lo[a] <= R.g0[a] and R.g1[a] <= hi[a] <= R.stored_hi[a] for a in range(3)), (cid, ring, R.rank, out)
            assert all(lo[a] <= max(R.g0[a] - st.halo, 0) and hi[a] >= min(R.g1[a] + st.halo, R.dims[a]) for a in range(3)), (cid, ring, R.rank, out)
            n += 1
    assert n > 200


def test_on_uploaded_sources_the_model_is_the_shard_rule(smk):
    """every single-link case of tests/_step_shard_ref.py: an upload, then one stencil"""
    for kind, dims, nranks, halo in S.CASES:
        for ring in S.RINGS:
            for r in range(nranks):
                R = C.Rank(dims, r, nranks, halo, ring)
                st = C.run(R, (("upload", 1, 0), ("stencil", 2, kind, 1)))
                assert st[1].box == S.uploaded_valid(dims, R.O, R.D)
                assert st[2].box == S.valid_box(dims, R.O, R.D, S.REACH[kind]), (kind, dims, nranks, halo, ring, r)
                assert st[2].halo == S.valid_halo_after(nranks, halo, S.REACH[kind])
                assert not C.telling_faces(R, st[2])


def test_on_dense_blocks_the_model_is_the_block_rule(smk):
    """every single-link case of tests/_step_block_ref.py, all three cuts: C, the halo rule and the stencil's valid box"""
    n = 0
    for case, (kind, dims, nranks, halo) in enumerate(B.CASES):
        for ring in B.RINGS:
            for which in B.CUTS:
                for c in B.cuts_of(case, ring, which):
                    R = C.Rank(dims, c.rank, nranks, c.option_halo, ring)
                    b = C.Block(R, c.origin, c.size)
                    assert (b.lo, b.hi) == (c.lo, c.hi) and b.halo == c.src_halo
                    assert C.box_of(C.erode(b.mask(), c.reach)) == (c.vlo, c.vhi), (kind, dims, ring, which, c.rank)
                    n += 1
    assert n > 200


def test_the_shard_rule_for_a_source_with_a_rim_is_the_models(smk):
    """tests/_step_shard_ref.valid_box(..., src=...) at every sharded stencil link of every chain case: a source that is not
    valid up to a face of the volume loses the reach there, wherever the stored box ends"""
    for cid, ring, R, links, steps in every_rank():
        for out, st in steps.items():
            if st.link[0] == "stencil":
                got = S.valid_box(R.dims, R.O, R.D, C.REACH[st.link[2]], src=C.box_of(st.src))
                assert got == st.box, "%s %s rank %d step %d: the shard rule gives %s, the erosion %s (telling faces %s)" % (
                    cid, ring, R.rank, out, got, st.box, C.telling_faces(R, st))


def test_every_case_has_a_telling_face():
    seen = set()
    for case, (cid, dims, nranks, halo, links) in enumerate(C.CASES):
        for ring in C.RINGS:
            faces = []
            for R in C.ranks_of(case, ring):
                steps = C.run(R, links)
                for st in steps.values():
                    for a, side in C.telling_faces(R, st):
                        faces.append((a, side))
                        seen.add((a, side, C.REACH[st.link[2]]))
                        layers = C.between(R, st, (a, side))
                        assert layers.any() and not (layers & st.mask).any() and not (layers & ~st.src).any()
                        assert layers.sum() % C.REACH[st.link[2]] == 0
            if cid in C.NO_TELLING_FACE:
                assert not faces and links[0][0] == "upload" and not any(l[0].startswith("block") for l in links), cid
            else:
                assert faces, "%s %s: no rank has a telling face" % (cid, ring)
    axes, sides, reaches = {f[0] for f in seen}, {f[1] for f in seen}, {f[2] for f in seen}
    assert axes == {0, 1, 2} and sides == {0, 1} and reaches == {1, 2}, seen
    assert len(C.NO_TELLING_FACE) == 1


def test_the_witness_has_two_rank_cases_of_each_reach():
    reaches = set()
    for case, (cid, dims, nranks, halo, links) in enumerate(C.CASES):
        if nranks != 2:
            continue
        for R in C.ranks_of(case, "u8"):
            for st in C.run(R, links).values():
                if C.telling_faces(R, st):
                    reaches.add(C.REACH[st.link[2]])
    assert reaches == {1, 2}


def test_every_link_has_the_halo_it_needs():
    for cid, ring, R, links, steps in every_rank():
        assert set(steps) == {l[1] for l in links}
        for out, st in steps.items():
            if st.need:
                assert st.need[0] >= st.need[1], (cid, ring, R.rank, out, st.need)
        assert steps[C.final(links)].halo >= 1, (cid, ring, R.rank)
        # the header's numbers: option halo, the block's, less the reach, the smaller of two
        for out, st in steps.items():
            what = st.link[0]
            if what == "upload":
                assert st.halo == R.option_halo
            elif what == "block":
                assert st.halo == st.link[3] < R.option_halo, "ghosts narrower than option halo"
            elif what == "block_stencil":
                assert st.halo == st.link[3] - C.REACH[st.link[2]]
            elif what == "blend":
                assert st.halo == min(steps[st.link[2]].halo, steps[st.link[3]].halo)
            else:
                assert st.halo == steps[st.link[3]].halo - C.REACH[st.link[2]]


def test_the_refused_chains_run_out_of_halo():
    for cid, dims, nranks, halo, links, refused, (have, reach) in C.REFUSED:
        for ring in C.RINGS:
            for r in range(nranks):
                R = C.Rank(dims, r, nranks, halo, ring)
                steps = C.run(R, links)                     # (what comes before is allowed)
                assert steps[refused[3]].halo == have and reach == C.REACH[refused[2]] and have < reach + 1
                with pytest.raises(C.Refused) as e:
                    C.run(R, links + (refused,))
                assert (e.value.have, e.value.reach, e.value.link) == (have, reach, refused)
    # an unsharded context has no halo to lose
    one = C.Rank((21, 9, 13), 0, 1, 1, "u8")
    st = C.run(one, C.REFUSED[0][4] + (C.REFUSED[0][5],))
    assert all(s.box == ((0, 0, 0), (21, 9, 13)) and s.halo == 1 for s in st.values())


def test_the_cases_cover_the_ground(smk):
    kinds, what, chains = set(), set(), {c[0].split("-")[0] for c in C.CASES}
    for cid, dims, nranks, halo, links in C.CASES:
        what |= {l[0] for l in links}
        kinds |= {l[2] for l in links if l[0] in ("stencil", "block_stencil")}
        assert int(np.prod(dims)) < 12000, "a few thousand voxels"
    assert what == {"upload", "block", "block_stencil", "blend", "stencil"} and kinds == {"derive", "merge"}
    assert chains == {"A", "B", "C", "D", "D2", "E", "F"} and set(C.RINGS) == {"u8", "u16", "f32"}
    assert {c[2] for c in C.CASES} == {2, 4, 8}
    # an odd x origin that the 8-byte evening made, and a stored box wider than a derive tile in x, on ranks with telling faces
    odd = wide = False
    for case, (cid, dims, nranks, halo, links) in enumerate(C.CASES):
        for R in C.ranks_of(case, "u8"):
            told = any(C.telling_faces(R, st) for st in C.run(R, links).values())
            odd |= told and R.O[0] % 2 == 1 and R.O[0] != max(R.g0[0] - halo, 0)
            wide |= told and R.D[0] > S.DERIVE_TILE[0] and final_is(links, "derive")
    assert odd and wide
    # a second stencil whose source has a rim of its own, with and without a telling face
    assert sum(len(C.stencil_links(c[4])) == 2 for c in C.CASES) == 2
    # a blend whose sources are valid on different boxes
    differ = False
    for R in C.ranks_of(C.CASE_IDS.index("F-merge-9x11x13-r2-h4"), "u8"):
        st = C.run(R, C.CHAIN_F)
        differ |= st[1].box != st[2].box and st[3].box == st[2].box
    assert differ


def final_is(links, kind):
    return C.final_kind(links) == kind


def test_a_block_takes_its_part_of_the_whole_array(smk):
    R = C.Rank((9, 11, 13), 1, 2, 4, "u8")
    b = R.block(2)
    assert (R.g0, R.g1) == ((4, 0, 0), (9, 11, 13)) and R.stored_lo[0] == 0 and (b.origin, b.size) == ((2, 0, 0), (7, 11, 13))
    assert (b.lo, b.hi) == ((2, 0, 0), (9, 11, 13)) and b.halo == 2
    whole = np.arange(9 * 11 * 13, dtype=np.float32).reshape(13, 11, 9)
    assert np.array_equal(b.take(whole), whole[:, :, 2:]) and b.mask().sum() == 7 * 11 * 13
