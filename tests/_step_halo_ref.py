"""The geometry of the halo refill (smk.h: smk_step_halo_layout, smk_step_halo_exports_device, smk_step_halo_entries_device,
smk_step_halo_exchange_local), restated in NumPy: the box every rank stores cut at the volume, the segments region_r ∩ S_j, their
byte counts and their places in a rank's exports and entries.  No GPU here; tests/test_step_halo_cpu.py qualifies the case
list so that no GPU test can pass vacuously.

Expected VOXELS never come from here: tests/test_gpu_step_halo.py takes them from sharded contexts that UPLOADED the unsharded
result.  The stored box is tests/_step_shard_ref.py's.  Volumes are [z][y][x]; dims, origins and sizes are (x, y, z)."""
import numpy as np

import _step_shard_ref as S

# a voxel class: (ring, nelts, normals) -> what decides the stored box (the ring), VB and NB
CLASSES = {
    "u8": ("u8", 3, True),
    "u16": ("u16", 3, True),
    "f32x3": ("f32", 3, True),      # the normal rides in .w
    "f32x4n": ("f32", 4, True),     # the separate normals buffer: NB = 4
    "f32x4": ("f32", 4, False),     # four channels and no normals: no buffer, NB = 0
}


def voxel_bytes(cls):
    """(VB, NB) of a class"""
    ring, nelts, normals = CLASSES[cls]
    return (16 if ring == "f32" else 8), (4 if ring == "f32" and nelts == 4 and normals else 0)


def roundup16(b):
    return (b + 15) // 16 * 16


def rank_boxes(dims, nranks, halo, ring):
    """per rank (g0, g1, s0, s1, pad): the region, and S = the stored box cut at the volume"""
    out = []
    for r in range(nranks):
        g0, g1, O, D, pad = S.stored_box(dims, r, nranks, halo, ring)
        out.append((g0, g1, tuple(O), tuple(min(o + d, n) for o, d, n in zip(O, D, dims)), pad))
    return out


def segment(boxes, r, j):
    """segment r -> j: the box (lo, hi) region_r ∩ S_j, or None when it is empty or r == j"""
    if r == j:
        return None
    lo = tuple(max(a, b) for a, b in zip(boxes[r][0], boxes[j][2]))
    hi = tuple(min(a, b) for a, b in zip(boxes[r][1], boxes[j][3]))
    return (lo, hi) if all(h > l for l, h in zip(lo, hi)) else None


def nvox(box):
    return 0 if box is None else int(np.prod([h - l for l, h in zip(*box)]))


def segment_bytes(n, cls):
    VB, NB = voxel_bytes(cls)
    return roundup16(n * VB) + roundup16(n * NB)


def layout(dims, nranks, halo, cls, r):
    """(send_bytes [P], recv_bytes [P], total_send, total_recv) of rank r"""
    boxes = rank_boxes(dims, nranks, halo, CLASSES[cls][0])
    send = [segment_bytes(nvox(segment(boxes, r, j)), cls) for j in range(nranks)]
    recv = [segment_bytes(nvox(segment(boxes, i, r)), cls) for i in range(nranks)]
    return send, recv, sum(send), sum(recv)


def offsets(counts):
    """where each segment starts: the exclusive prefix sums of the byte counts"""
    return [int(x) for x in np.concatenate([[0], np.cumsum(counts)[:-1]])]


def segment_kind(box, region):
    """how many axes the segment is cut on against the owner's region: 1 a face, 2 an edge, 3 a corner (0: the whole region)"""
    return sum(1 for a in range(3) if (box[1][a] - box[0][a]) < (region[1][a] - region[0][a]))


# ---- the cases: (dims, nranks, halo); tests/test_step_halo_cpu.py says what they cover
CASES = (
    ((21, 13, 11), 2, 3),      # rank 1's x origin is odd (7); rank 0's 8-byte rows are evened by one more halo voxel
    ((22, 13, 11), 2, 3),      # rank 1's x origin is even (8)
    ((22, 13, 11), 4, 4),      # rank 1's 8-byte rows end on the volume's face: evened by a moved origin (7 -> 6)
    ((21, 13, 11), 8, 3),      # every axis split: face, edge and corner segments
    ((21, 13, 11), 4, 7),      # halo 7 >= the 6 and 7 rows of the y regions: S spans y, with a pad row
    ((21, 13, 11), 2, 11),     # halo 11 >= rank 1's 11 columns: rank 0 stores all of x, with a pad column
    ((22, 13, 11), 8, 7),      # S spans y and z on every rank
)
CASE_IDS = ["%s-r%d-h%d" % ("x".join(map(str, d)), n, h) for d, n, h in CASES]
