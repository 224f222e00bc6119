"""The merge with H and blurred normals on a shard and from blocks (smk.h: smk_step_extremes_h_device,
smk_merge_timestep_h_shard, smk_block_extremes_h_device, smk_upload_timestep_fields_h_block_device), restated in NumPy: the
cases, the eight words a region exports, and what the stencil makes of a stored box whose surroundings are zeros -- the reason
the reach is 2.  No GPU here; tests/test_step_merge_h_shard_cpu.py qualifies all of it so that no GPU test can pass vacuously.

Expected VOXELS never come from here: tests/test_gpu_step_merge_h_shard.py takes them from the one-call entries on an
unsharded context in the same test.  The stored box, the valid box and the ordered integers are tests/_step_shard_ref.py's,
the arithmetic tests/_step_merge_h_ref.py's.  Volumes are [z][y][x]; dims, origins and sizes are (x, y, z)."""
import numpy as np

import _prep_f32_ref as P
import _step_merge_h_ref as H
import _step_shard_ref as S
from _step_shard_ref import stored_box, valid_box, in_box, cells_of, ordered, combine, place, INT_MIN  # noqa: F401

F32 = np.float32
REACH = 2                                                   # for every (add_h, blur): the apron of F (csrc/smk_step_merge_h.hip)
TILE = H.TILE
RINGS = H.RINGS
BLUR_ONLY = {"u8": 3, "u16": 2, "f32": 3}                   # nf of the layouts that have no room for H: add_h 0

# (dims, ranks, halo): the derive's shapes, the smallest at which a 32 x 8 x 8 tile with a 2-voxel apron can still go wrong
CASES = (
    ((75, 21, 19), 2, 3),      # an odd x origin on rank 1; a stored box wider than a tile, thicker than 8 in y and z
    ((74, 21, 19), 4, 4),      # an even x origin; y split
    ((75, 21, 19), 8, 3),      # every axis split
    ((7, 9, 11), 2, 3),        # all odd; rank 1 stores all of x with a pad column, rank 0 stops short without one
    ((3, 21, 19), 2, 3),       # 3 voxels along the split axis: rank 0's region is border voxels alone and exports the seeds
)
CASE_IDS = ["%s-r%d-h%d" % ("x".join(map(str, d)), n, h) for d, n, h in CASES]

# the seed of a case's fields.  Cases 0 to 2: the first under which, for every ring, every nf of a V1GH / V2GH layout and both
# values of compat, every rank's words differ from the combined ones in one of the three, so that the extremes are not all
# attained in rank 0's region (qualified in the CPU test).  The small volumes of cases 3 and 4 are not held to that: in the
# last one a single rank has interior voxels at all
SEED = {0: 9, 1: 1, 2: 0, 3: 0, 4: 0}

WORD_SEEDS = np.array([0, ~S.ORD_POS_INF, S.ORD_NEG_INF] + [INT_MIN] * 5, np.int32)


def layouts(case, ring):
    """the (nf, add_h, blur, compat) a case runs in a ring: every flag combination on the first case, (1, 1, 1) and (0, 1, 1)
    on the others; nf as _step_merge_h_ref.NFS with H, and the blur-only layouts without"""
    top = H.NFS[ring][-1]
    if case == 0:
        out = [(top if a or not b else BLUR_ONLY[ring], a, b, c) for a, b, c in H.FLAGS]
        out += [(nf, 1, 1, 1) for nf in H.NFS[ring][:-1]] + [(top, 0, 1, 1)]
    else:
        out = [(nf, 1, 1, 1) for nf in H.NFS[ring]] + [(BLUR_ONLY[ring], 0, 1, 1)]
    return out


def fields(case, ring, nf):
    return H.fields(ring, nf, CASES[case][0], SEED[case])


def source(case, ring, nf, add_h):
    """a resident step that holds the case's fields: (data [z][y][x][nf + 1 + add_h], normals)"""
    return H.source_step(fields(case, ring, nf), add_h)


# ---- the words

def unscaled(F, compat):
    """(|S| [z][y][x], hs [z][y][x], the blurred normal bytes, the plain ones) of fields F over the array they come in: the
    border is the ARRAY's, which is the volume's when F is volume-sized"""
    Sg = H.summed(np.ascontiguousarray(F).astype(F32))
    with np.errstate(all="ignore"):
        mag = np.sqrt(Sg[..., 0] * Sg[..., 0] + Sg[..., 1] * Sg[..., 1] + Sg[..., 2] * Sg[..., 2])
    return mag, H.second_derivative(Sg, compat), P.normal_bytes(P.blur_gradient(Sg)), P.normal_bytes(Sg)


def region_words(F, g0, g1, add_h, compat):
    """the eight words region [g0, g1) of the volume-sized fields F exports: what pass 1 counts over the region's interior
    voxels of the volume"""
    flt = H.RING_OF[np.ascontiguousarray(F).dtype] != "u8"
    mag, hs, _, _ = unscaled(F, compat)
    nz, ny, nx = mag.shape
    sl = tuple(slice(max(g0[a], 1), min(g1[a], n - 1)) for a, n in ((2, nz), (1, ny), (0, nx)))
    w = WORD_SEEDS.copy()
    m = mag[sl].ravel()
    m = m[np.isfinite(m)] if flt else m
    if m.size:
        w[0] = max(0, int(ordered(m).max()))
    if add_h:
        h = hs[sl].ravel()
        h = h[np.isfinite(h) if flt else ~np.isnan(h)]
        if h.size:
            o = ordered(h)
            w[1], w[2] = ~int(o.min()), int(o.max())
    return w


def words_extremes(w):
    """(max magnitude, min H, max H) of words as floats"""
    w = np.asarray(w, np.int32)
    return float(S.unordered(w[0])), float(S.unordered(~w[1])), float(S.unordered(w[2]))


# ---- the witness: why the reach is 2

def zeroed_outside(F, lo, hi):
    """F with zeros outside the global box [lo, hi): what a context that stores that box holds in F's LDS tile"""
    out = np.zeros_like(F)
    out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = F[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    return out


def cut_distance(dims, lo, hi):
    """[z][y][x] over the volume: inside the box [lo, hi) the distance of a voxel to the nearest face of the box that is no
    face of the volume (0: the voxel lies on it), a large number when the box has no such face; -1 outside the box"""
    big = 10 ** 6
    d = np.full(dims[::-1], big, np.int64)
    for a, ax in ((0, 2), (1, 1), (2, 0)):
        g = np.arange(dims[a])
        da = np.full(dims[a], big, np.int64)
        if lo[a] > 0:
            da = np.minimum(da, g - lo[a])
        if hi[a] < dims[a]:
            da = np.minimum(da, hi[a] - 1 - g)
        d = np.minimum(d, da.reshape([-1 if i == ax else 1 for i in range(3)]))
    d[~in_box(dims[::-1], (0, 0, 0), lo, hi)] = -1
    return d


def same_bits(a, b):
    """elementwise: the same bits (a NaN equals itself, -0 differs from +0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a == b
