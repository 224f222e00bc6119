"""The geometry of the block entries (smk.h: smk_block, smk_declare_volume, smk_upload_timestep_block_device,
smk_block_extremes_device, smk_upload_timestep_scalar_block_device, smk_upload_timestep_fields_block_device), restated in
NumPy: C = block ∩ stored box ∩ volume, the valid box of a result, the halo rule, and the three cuts of the whole arrays every
rank's block comes in.  No GPU here; tests/test_step_block_cpu.py qualifies the case list so that no GPU test can pass
vacuously.

Expected VOXELS never come from here: tests/test_gpu_step_block.py takes them from the one-call entries on an unsharded
context in the same test.  The cases, the stored box, the words and the placement are tests/_step_shard_ref.py's.
Volumes are [z][y][x]; dims, origins and sizes are (x, y, z)."""
import numpy as np

import _step_shard_ref as S
from _step_shard_ref import CASES, CASE_IDS, RINGS, REACH, SEEDS, INT_MIN, M, stored_box, combine, place  # noqa: F401

CUTS = ("a", "b", "c")
WIDER = 2                                                   # cut (c): option halo = the case's + WIDER


def intersect(lo_a, hi_a, lo_b, hi_b):
    return tuple(max(a, b) for a, b in zip(lo_a, lo_b)), tuple(min(a, b) for a, b in zip(hi_a, hi_b))


def c_box(dims, origin, size, O, D):
    """C: block ∩ stored box ∩ volume, as (lo, hi) in global voxels"""
    lo, hi = intersect(origin, tuple(o + s for o, s in zip(origin, size)), O, tuple(o + d for o, d in zip(O, D)))
    return intersect(lo, hi, (0, 0, 0), dims)


def contains(lo, hi, g0, g1):
    return all(lo[a] <= g0[a] and g1[a] <= hi[a] for a in range(3))


def source_halo(dims, g0, g1, lo, hi, halo):
    """the smallest number of voxels C extends beyond the region over the region's faces that are no faces of the volume,
    capped at option halo.  Where C reaches the volume's own face, no voxel lies beyond it: that side gives all a halo can
    (the 3-voxel-thick cases: rank 1's region [1, 3) has one voxel before it, and it is the volume's first)"""
    h = halo
    for a in range(3):
        if g0[a] > 0 and lo[a] > 0:
            h = min(h, g0[a] - lo[a])
        if g1[a] < dims[a] and hi[a] < dims[a]:
            h = min(h, hi[a] - g1[a])
    return h


def valid_box(dims, lo, hi, reach):
    """C shrunk by the reach at every face of C that is no face of the volume"""
    return (tuple(lo[a] if lo[a] == 0 else lo[a] + reach for a in range(3)),
            tuple(hi[a] if hi[a] >= dims[a] else hi[a] - reach for a in range(3)))


def result_halo(nranks, have, reach):
    return have - reach if nranks > 1 else have


def grown(dims, g0, g1, m):
    """the region ± m voxels, cut at the volume, as (origin, size)"""
    lo = tuple(max(g0[a] - m, 0) for a in range(3))
    hi = tuple(min(g1[a] + m, dims[a]) for a in range(3))
    return lo, tuple(h - l for l, h in zip(lo, hi))


class Cut:
    """one rank's block in one cut of the whole arrays"""

    def __init__(self, kind, dims, rank, nranks, halo, ring, which, reach=None):
        reach = REACH[kind] if reach is None else reach
        self.which, self.dims, self.rank, self.nranks, self.reach = which, dims, rank, nranks, reach
        self.option_halo = halo + WIDER if which == "c" else halo
        self.g0, self.g1, self.O, self.D, self.pad = stored_box(dims, rank, nranks, self.option_halo, ring)
        if which == "a":                                    # region ± option halo: narrower than the stored box where a row was evened
            self.origin, self.size = grown(dims, self.g0, self.g1, halo)
        elif which == "b":                                  # a pitched view of the whole volume's array: what of it the box stores
            self.origin = self.O
            self.size = tuple(min(o + d, n) - o for o, d, n in zip(self.O, self.D, dims))
        else:                                               # region ± (reach + 1) under a larger option halo
            self.origin, self.size = grown(dims, self.g0, self.g1, max(reach, 0) + 1)
        self.view = which == "b"
        self.lo, self.hi = c_box(dims, self.origin, self.size, self.O, self.D)
        self.src_halo = source_halo(dims, self.g0, self.g1, self.lo, self.hi, self.option_halo)
        self.vlo, self.vhi = valid_box(dims, self.lo, self.hi, max(reach, 0))
        self.halo = result_halo(nranks, self.src_halo, max(reach, 0))
        self.stored_lo, self.stored_hi = S.uploaded_valid(dims, self.O, self.D)

    def rim(self):
        """bool over the stored box cut at the volume: the voxels outside the result's valid box"""
        shape = tuple(h - l for l, h in zip(self.stored_lo, self.stored_hi))[::-1]
        return ~S.in_box(shape, self.stored_lo, self.vlo, self.vhi)

    def take(self, whole, poison=None):
        """(array to hand over, offset in ELEMENTS of the block's first element, pitch_y, pitch_z) of this cut of `whole`
        [z][y][x](...).  A view: a copy of the whole array, everything outside the view overwritten with `poison`"""
        (ox, oy, oz), (sx, sy, sz) = self.origin, self.size
        if not self.view:
            return np.ascontiguousarray(whole[oz:oz + sz, oy:oy + sy, ox:ox + sx]), 0, 0, 0
        nz, ny, nx = whole.shape[:3]
        a = np.empty_like(whole)
        a[...] = poison
        a[oz:oz + sz, oy:oy + sy, ox:ox + sx] = whole[oz:oz + sz, oy:oy + sy, ox:ox + sx]
        return a, (oz * ny + oy) * nx + ox, nx, nx * ny


def cuts_of(case, ring, which, reach=None):
    kind, dims, nranks, halo = CASES[case]
    return [Cut(kind, dims, r, nranks, halo, ring, which, reach) for r in range(nranks)]


POISON = {"u8": 0xA5, "u16": 0xA5A5, "f32": np.float32(-7.0e30)}


def scalar(ring, dims, seed=0):
    """a dense scalar [z][y][x] of a type"""
    return np.ascontiguousarray(M.fields(ring, 1, dims, seed)[..., 0])


def region_words(kind, F, g0, g1):
    """what can be said in NumPy of the words region [g0, g1) of fields F [z][y][x][nf] exports, in the shard reference's
    encoding (derive_words, merge_words): the derive's V words of channel 0 -- its G and H words left at their seeds: their
    arithmetic is the entries', which no test restates --, the merge's one word; the seeds from a region without an interior
    voxel"""
    nz, ny, nx = F.shape[:3]
    sl = tuple(slice(max(g0[a], 1), min(g1[a], n - 1)) for a, n in ((2, nz), (1, ny), (0, nx)))
    if kind == "derive":
        v = F[..., 0][sl].astype(np.float32)
        return S.derive_words(v.min(), v.max(), np.inf, -np.inf, np.inf, -np.inf) if v.size else SEEDS[kind].copy()
    mag = M.magnitude(F)[sl]
    return S.merge_words(mag.max()) if mag.size else SEEDS[kind].copy()
