"""The geometry and the words of the stencil producers on a shard (smk.h: smk_step_extremes_device, smk_derive_timestep_shard,
smk_merge_timestep_shard), restated in NumPy: the box a sharded context stores, the valid box of a derived or merged step, its
rim, and the eight words the ranks exchange.  No GPU here; tests/test_step_shard_cpu.py qualifies the case list so that no
GPU test can pass vacuously.

Expected VOXELS never come from here: tests/test_gpu_step_shard.py takes them from the one-call entries on an unsharded
context in the same test.  Volumes are [z][y][x]; dims, origins and sizes are (x, y, z)."""
import numpy as np

import _step_merge_ref as M

REACH = {"derive": 2, "merge": 1}
DERIVE_TILE = (32, 8, 8)                                    # DV_TX, DV_TY, DV_TZ (csrc/smk_step_derive.hip), voxels
MERGE_TILE_X = {"u8": 128, "u16": 128, "f32": 64}           # MG_UX units of two 8-byte voxels or one f32 voxel
INT_MIN = -2 ** 31


# ---- the stored box (smk_volume_geometry) and the valid box

def stored_box(dims, rank, nranks, halo, ring):
    """(g0, g1, O, D, pad): the region, the stored box of D voxels from voxel O, and per axis whether its last column or row
    is a pad behind the volume.  The region plus `halo` voxels, cut at the volume; rows of 8-byte voxels are then made even in
    x and y: by one more voxel where the volume has one, else by one before the box, else by a pad."""
    from conftest import load_package
    load_package()
    from simian_spacemonkey_amd import sortlast
    g0, g1 = sortlast.shard_region(dims, rank, nranks)     # (the mirror of the C++ shard rule)
    O, D, pad = [0] * 3, [0] * 3, [False] * 3
    for a in range(3):
        lo, hi = max(g0[a] - halo, 0), min(g1[a] + halo, dims[a])
        O[a], D[a] = lo, hi - lo
    if ring != "f32":
        for a in range(2):
            if D[a] & 1:
                if O[a] + D[a] < dims[a]:
                    D[a] += 1
                elif O[a] > 0:
                    O[a] -= 1
                    D[a] += 1
                else:
                    D[a] += 1
                    pad[a] = True
    return tuple(g0), tuple(g1), tuple(O), tuple(D), tuple(pad)


def uploaded_valid(dims, O, D):
    """the valid box (lo, hi) of an uploaded step: the stored box cut at the volume"""
    return tuple(O), tuple(min(o + d, n) for o, d, n in zip(O, D, dims))


def valid_box(dims, O, D, reach, src=None):
    """the valid box (lo, hi), global voxels, of a stencil of `reach` over a source whose valid box is `src` (None: an
    upload's): the source's shrunk by `reach` at every face of it that is not a face of the volume.  An upload's valid box is
    the stored box cut at the volume, so for an upload these are the faces of the stored box"""
    slo, shi = src or uploaded_valid(dims, O, D)
    lo = tuple(slo[a] if slo[a] == 0 else slo[a] + reach for a in range(3))
    hi = tuple(shi[a] if shi[a] >= dims[a] else shi[a] - reach for a in range(3))
    return lo, hi


def cut_anywhere(dims, O, D):
    return any(O[a] != 0 or O[a] + D[a] < dims[a] for a in range(3))


def valid_halo_after(nranks, have, reach):
    """the valid halo of the result: the source's less the reach on every rank of a sharded series, unchanged without shards"""
    return have - reach if nranks > 1 else have


def in_box(shape_zyx, O, lo, hi):
    """bool [z][y][x] over a box stored from O: the voxels inside the global box [lo, hi)"""
    m = np.ones(shape_zyx, bool)
    for a, ax in ((0, 2), (1, 1), (2, 0)):
        g = O[a] + np.arange(shape_zyx[ax])
        sel = (g >= lo[a]) & (g < hi[a])
        m &= sel.reshape([-1 if i == ax else 1 for i in range(3)])
    return m


def cells_of(lo, hi):
    """every probe cell (x, y, z of its low corner) whose eight corners lie in the box [lo, hi)"""
    r = [np.arange(lo[a], hi[a] - 1) for a in range(3)]
    x, y, z = np.meshgrid(r[0], r[1], r[2], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], -1).astype(np.int32)


def straddles(cells, g0, g1):
    """the cells that have a corner inside the region [g0, g1) and a corner outside it"""
    any_in = np.zeros(len(cells), bool)
    all_in = np.ones(len(cells), bool)
    for d in np.ndindex(2, 2, 2):
        c = cells + np.array(d)
        i = np.all((c >= np.array(g0)) & (c < np.array(g1)), -1)
        any_in |= i
        all_in &= i
    return any_in & ~all_in


def has_interior(dims, g0, g1):
    """the region holds a voxel that is off the volume's 1-voxel border"""
    return all(max(g0[a], 1) < min(g1[a], dims[a] - 1) for a in range(3))


# ---- the words

def ordered(x):
    """the ordered int of a float32: ascending with the float"""
    b = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, b ^ 0x7fffffff).astype(np.int32)


def unordered(i):
    i = np.asarray(i, np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7fffffff).astype(np.int32).view(np.float32)


ORD_POS_INF, ORD_NEG_INF = int(ordered(np.inf)), int(ordered(-np.inf))
DERIVE_SEEDS = np.array([~ORD_POS_INF, ORD_NEG_INF] * 3 + [INT_MIN] * 2, np.int32)
MERGE_SEEDS = np.array([0] + [INT_MIN] * 7, np.int32)
SEEDS = {"derive": DERIVE_SEEDS, "merge": MERGE_SEEDS}


def derive_words(vmin, vmax, gmin, gmax, hmin, hmax):
    w = DERIVE_SEEDS.copy()
    for k, (lo, hi) in enumerate(((vmin, vmax), (gmin, gmax), (hmin, hmax))):
        w[2 * k], w[2 * k + 1] = ~int(ordered(lo)), int(ordered(hi))
    return w


def derive_extremes(w):
    """(vmin, vmax, gmin, gmax, hmin, hmax) of derive words"""
    w = np.asarray(w, np.int32)
    return tuple(float(unordered(~w[k] if k % 2 == 0 else w[k])) for k in range(6))


def merge_words(mx):
    w = MERGE_SEEDS.copy()
    w[0] = int(ordered(mx))
    return w


def combine(words):
    """the ranks' words [P][8] -> the words every rank writes with: the elementwise integer maximum"""
    return np.asarray(words, np.int32).reshape(-1, 8).max(0)


# ---- the cases: (kind, dims, nranks, halo).  Each ring runs each (tests/test_step_shard_cpu.py says what they cover)

CASES = (
    ("derive", (75, 21, 19), 2, 3),    # an odd x origin on rank 1; a stored box wider than a derive tile, thicker than 8 in y and z
    ("derive", (74, 21, 19), 4, 4),    # an even x origin; y split
    ("derive", (75, 21, 19), 8, 3),    # every axis split
    ("derive", (7, 9, 11), 2, 3),      # all odd; rank 1 stores all of x with a pad column, rank 0 stops short without one
    ("derive", (3, 21, 19), 2, 3),     # 3 voxels along the split axis: rank 0's region is border voxels alone
    ("merge", (263, 9, 7), 2, 2),      # a stored box wider than one tile row of the merge kernels
    ("merge", (74, 21, 19), 4, 3),
    ("merge", (75, 21, 19), 8, 2),
    ("merge", (3, 21, 19), 2, 2),
)
RINGS = ("u8", "u16", "f32")
CASE_IDS = ["%s-%s-r%d-h%d" % (k, "x".join(map(str, d)), n, h) for k, d, n, h in CASES]


def source(kind, ring, dims, nf=2, seed=0):
    """a resident step the producers read: (data [z][y][x][nelts], normals).  Derive: three channels, channel 0 the scalar;
    merge: nf fields and a last channel.  The last channel and the normals are NOT what the producers make."""
    if kind == "derive":
        nf = 2
    return M.source_step(M.fields(ring, nf, dims, seed), seed + 5)


def place(dims, nelts, dtype, parts):
    """the ranks' region downloads ((origin, data) each) placed at their origins in a volume-sized array"""
    nx, ny, nz = dims
    out = np.zeros((nz, ny, nx, nelts), dtype)
    seen = np.zeros((nz, ny, nx), np.int32)
    for (ox, oy, oz), d in parts:
        sz, sy, sx = d.shape[:3]
        out[oz:oz + sz, oy:oy + sy, ox:ox + sx] = d
        seen[oz:oz + sz, oy:oy + sy, ox:ox + sx] += 1
    assert (seen == 1).all(), "the regions do not tile the volume"
    return out
