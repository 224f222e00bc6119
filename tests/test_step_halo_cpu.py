"""tests/_step_halo_ref.py qualified (no GPU): for every receiver its region and the incoming segments tile the box it stores
exactly once, what r sends to j is what j receives from r, and the case list of tests/test_gpu_step_halo.py covers what the
gather and the scatter of sub-boxes can get wrong."""
import itertools

import numpy as np

import _step_halo_ref as HR
import _step_shard_ref as S

SWEEP_DIMS = ((21, 13, 11), (22, 13, 11), (7, 9, 11), (2, 2, 2), (3, 21, 19), (75, 21, 19), (16, 16, 16))
SWEEP_HALOS = (1, 2, 3, 4, 7, 11, 40)


def test_region_and_segments_tile_the_stored_box_exactly_once(smk):
    for dims, nranks, halo, ring in itertools.product(SWEEP_DIMS, (1, 2, 4, 8), SWEEP_HALOS, S.RINGS):
        boxes = HR.rank_boxes(dims, nranks, halo, ring)
        for j, (g0, g1, s0, s1, pad) in enumerate(boxes):
            seen = np.zeros(dims[::-1], np.int32)
            seen[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]] += 1
            for i in range(nranks):
                b = HR.segment(boxes, i, j)
                if b is None:
                    continue
                (x0, y0, z0), (x1, y1, z1) = b
                seen[z0:z1, y0:y1, x0:x1] += 1
                # the segment lies in the owner's region and outside the receiver's
                assert all(boxes[i][0][a] <= b[0][a] and b[1][a] <= boxes[i][1][a] for a in range(3))
                assert any(b[1][a] <= g0[a] or b[0][a] >= g1[a] for a in range(3))
            want = S.in_box(dims[::-1], (0, 0, 0), s0, s1).astype(np.int32)
            assert np.array_equal(seen, want), (dims, nranks, halo, ring, j)
            assert all(s1[a] <= dims[a] for a in range(3)), "the pad column lies outside the volume and outside S"


def test_what_r_sends_to_j_is_what_j_receives_from_r(smk):
    for dims, nranks, halo, cls in itertools.product(SWEEP_DIMS, (1, 2, 4, 8), SWEEP_HALOS, HR.CLASSES):
        lay = [HR.layout(dims, nranks, halo, cls, r) for r in range(nranks)]
        for r in range(nranks):
            send, recv, ts, tr = lay[r]
            assert send[r] == 0 and recv[r] == 0 and ts == sum(send) and tr == sum(recv)
            assert all(b % 16 == 0 for b in send + recv)
            for j in range(nranks):
                assert send[j] == lay[j][1][r], (dims, nranks, halo, cls, r, j)
        if nranks == 1:
            assert lay[0] == ([0], [0], 0, 0)
        # under the shard rule (two parts per axis, halo >= 1) every pair of ranks is adjacent: no segment between two
        # different ranks is empty, and the one empty segment of a rank is its own
        assert all(lay[r][0][j] > 0 for r in range(nranks) for j in range(nranks) if j != r)


def test_byte_counts_and_offsets():
    assert HR.voxel_bytes("u8") == (8, 0) and HR.voxel_bytes("u16") == (8, 0) and HR.voxel_bytes("f32x3") == (16, 0)
    assert HR.voxel_bytes("f32x4n") == (16, 4) and HR.voxel_bytes("f32x4") == (16, 0)
    assert HR.segment_bytes(0, "f32x4n") == 0
    assert HR.segment_bytes(3, "u8") == 32 and HR.segment_bytes(4, "u8") == 32          # (an odd count leaves 8 bytes unused)
    assert HR.segment_bytes(3, "f32x4n") == 48 + 16 and HR.segment_bytes(5, "f32x4n") == 80 + 32
    assert HR.offsets([32, 0, 48, 16]) == [0, 32, 32, 80]


def test_the_cases_cover_the_ground(smk):
    dims_seen = {(d, h) for d, _, h in HR.CASES}
    assert dims_seen >= {((21, 13, 11), 3), ((22, 13, 11), 3), ((21, 13, 11), 7), ((22, 13, 11), 7)}, "the smallest shapes and halos"
    assert {n for _, n, _ in HR.CASES} >= {2, 4, 8}
    par, extra, moved, padcol, padrow, spans, kinds, odd_rows = set(), False, False, False, False, set(), set(), False
    for dims, nranks, halo in HR.CASES:
        boxes8 = HR.rank_boxes(dims, nranks, halo, "u8")
        boxes16 = HR.rank_boxes(dims, nranks, halo, "f32")
        for r, ((g0, g1, s0, s1, pad), wide) in enumerate(zip(boxes8, boxes16)):
            if s0[0] > 0:
                par.add(s0[0] % 2)
            for a in range(2):
                extra |= s1[a] == wide[3][a] + 1                                        # one more halo voxel than the f32 box keeps
                moved |= s0[a] == wide[2][a] - 1                                        # ... or one before it
            padcol |= pad[0]
            padrow |= pad[1]
            for a in range(3):
                if (s0[a], s1[a]) == (0, dims[a]) and (g0[a], g1[a]) != (0, dims[a]):
                    other = dims[a] - (g1[a] - g0[a])
                    assert halo >= other, "S spans a split axis only when the halo covers the neighbour's region"
                    spans.add(a)
            for j in range(nranks):
                b = HR.segment(boxes8, r, j)
                if b is not None:
                    kinds.add(HR.segment_kind(b, (g0, g1)))
                    odd_rows |= (b[1][0] - b[0][0]) % 2 == 1 and (b[1][1] - b[0][1]) > 1  # rows of a packed segment change parity
    assert par == {0, 1}, "both parities of a rank's x origin"
    assert extra and moved, "a stored box evened by one more halo voxel, and one by a moved origin"
    assert padcol and padrow, "a pad column and a pad row"
    assert spans >= {0, 1, 2}, "a halo at least as large as a neighbour's region, on every axis"
    assert kinds >= {1, 2, 3}, "face, edge and corner segments"
    assert odd_rows
    assert S.stored_box((21, 13, 11), 1, 2, 3, "u8")[2][0] == 7 and S.stored_box((22, 13, 11), 1, 2, 3, "u8")[2][0] == 8
    assert S.stored_box((22, 13, 11), 1, 4, 4, "u8")[2][0] == 6 and S.stored_box((22, 13, 11), 1, 4, 4, "f32")[2][0] == 7
    assert S.stored_box((21, 13, 11), 0, 2, 11, "u8")[3:] == ((22, 14, 11), (True, True, False))
    # an empty segment: a rank's own (index r of its exports and entries); every class is a case of the GPU tests
    assert all(HR.layout(d, n, h, "u8", 0)[0][0] == 0 for d, n, h in HR.CASES)
    assert set(HR.CLASSES) == {"u8", "u16", "f32x3", "f32x4n", "f32x4"}
