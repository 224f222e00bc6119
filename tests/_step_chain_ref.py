"""What is valid of a resident step after a CHAIN of producers on a sharded context (smk.h: smk_upload_timestep*,
smk_upload_timestep_block_device, the block stencil forms, smk_blend_timesteps, smk_derive_timestep_shard,
smk_merge_timestep_shard), modelled in NumPy without any rule about faces: a step's validity is a boolean MASK over the
volume's voxels, and a stencil of reach r keeps a voxel when every voxel of the volume within r of it, per axis, is valid --
an erosion.  Positions outside the volume count as valid: nothing is there to know.  The box rules of tests/_step_shard_ref.py
and tests/_step_block_ref.py decide "a face of the volume" per face; this model never asks.  No GPU here;
tests/test_step_chain_cpu.py qualifies the model and the case list so that no GPU test can pass vacuously.

Expected VOXELS never come from here: tests/test_gpu_step_chain.py takes them from the same chain through the one-call
entries on an unsharded context.  The stored box is tests/_step_shard_ref.py's (qualified by tests/test_step_shard_cpu.py).
Volumes are [z][y][x]; dims, origins and sizes are (x, y, z).

A chain is a list of links over step ids (step 0 is the declared volume of zeros):
    ("upload", out, seed)                 the whole step `seed` through the upload entries
    ("block", out, seed, m)               the packed block form: the region +- m ghosts of step `seed`, cut at the volume
    ("block_stencil", out, kind, m)       the block stencil form from the dense fields of seed 0, region +- m ghosts
    ("blend", out, a, b, w)
    ("stencil", out, kind, src)           smk_step_extremes_device + smk_<kind>_timestep_shard"""
import numpy as np

import _step_shard_ref as S

REACH = S.REACH


# ---- masks

def box_mask(dims, lo, hi):
    """bool [z][y][x] over the volume: the voxels of the box [lo, hi) (cut at the volume)"""
    m = np.zeros(dims[::-1], bool)
    lo = [max(v, 0) for v in lo]
    hi = [min(v, n) for v, n in zip(hi, dims)]
    if all(a < b for a, b in zip(lo, hi)):
        m[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    return m


def erode(mask, r):
    """the voxels whose whole neighbourhood of +-r voxels per axis is valid; outside the volume everything is"""
    m = np.pad(mask, r, constant_values=True)
    for ax in range(3):                                     # (a box neighbourhood: one axis after the other)
        n = m.shape[ax] - 2 * r
        keep = np.ones([n if i == ax else s for i, s in enumerate(m.shape)], bool)
        for d in range(2 * r + 1):
            keep &= np.take(m, np.arange(d, d + n), axis=ax)
        m = keep
    assert m.shape == mask.shape
    return m


def box_of(mask):
    """(lo, hi) of a mask that is exactly one non-empty box, else None"""
    if not mask.any():
        return None
    z, y, x = np.nonzero(mask)
    lo, hi = (int(x.min()), int(y.min()), int(z.min())), (int(x.max()) + 1, int(y.max()) + 1, int(z.max()) + 1)
    return (lo, hi) if np.array_equal(mask, box_mask(mask.shape[::-1], lo, hi)) else None


# ---- one rank of a case

class Rank:
    def __init__(self, dims, rank, nranks, halo, ring):
        self.dims, self.rank, self.nranks, self.option_halo, self.ring = tuple(dims), rank, nranks, halo, ring
        self.g0, self.g1, self.O, self.D, self.pad = S.stored_box(dims, rank, nranks, halo, ring)
        self.stored_lo, self.stored_hi = tuple(self.O), tuple(min(o + d, n) for o, d, n in zip(self.O, self.D, dims))

    def stored(self):
        return box_mask(self.dims, self.stored_lo, self.stored_hi)

    def block(self, m):
        """a Block of the region +- m voxels, cut at the volume"""
        lo = tuple(max(g - m, 0) for g in self.g0)
        hi = tuple(min(g + m, n) for g, n in zip(self.g1, self.dims))
        return Block(self, lo, tuple(h - l for l, h in zip(lo, hi)))


class Block:
    """an array a rank hands over: `size` voxels from global voxel `origin`; C is what of it the context stores"""

    def __init__(self, rank, origin, size):
        self.rank, self.origin, self.size = rank, tuple(origin), tuple(size)
        R = rank
        self.lo = tuple(max(o, s, 0) for o, s in zip(origin, R.stored_lo))
        self.hi = tuple(min(o + n, s) for o, n, s in zip(origin, size, R.stored_hi))
        # the source's valid halo (smk.h, THE VALID BOX OF A BLOCK): the fewest voxels C extends beyond the region over the
        # region's faces that are no faces of the volume, capped at option halo; C on the volume's own face gives all
        h = R.option_halo
        if R.nranks > 1:
            for a in range(3):
                if R.g0[a] > 0 and self.lo[a] > 0:
                    h = min(h, R.g0[a] - self.lo[a])
                if R.g1[a] < R.dims[a] and self.hi[a] < R.dims[a]:
                    h = min(h, self.hi[a] - R.g1[a])
        self.halo = h

    def mask(self):
        return box_mask(self.rank.dims, self.lo, self.hi)

    def take(self, whole):
        """the block's own contiguous copy of `whole` [z][y][x](...)"""
        (ox, oy, oz), (sx, sy, sz) = self.origin, self.size
        return np.ascontiguousarray(whole[oz:oz + sz, oy:oy + sy, ox:ox + sx])


class Step:
    """what the model says of one step on one rank: its mask, its valid halo, and for the link that made it the source's mask
    (a stencil link), the block (a block link) and what the link needed of its source's valid halo: (have, need)"""

    def __init__(self, link, mask, halo, src=None, block=None, need=None):
        self.link, self.mask, self.halo, self.src, self.block, self.need = link, mask, halo, src, block, need

    @property
    def box(self):
        return box_of(self.mask)


class Refused(Exception):
    def __init__(self, link, have, reach):
        Exception.__init__(self, "%s: a valid halo of %d, the stencil reaches %d" % (link, have, reach))
        self.link, self.have, self.reach = link, have, reach


def run(R, links):
    """{step id: Step} of the chain on rank R.  Raises Refused at the first link whose source lacks the valid halo"""
    sharded = R.nranks > 1
    steps = {}
    for link in links:
        what, out = link[0], link[1]
        if what == "upload":
            st = Step(link, R.stored(), R.option_halo)
        elif what == "block":
            b = R.block(link[3])
            if sharded and b.halo < 1:
                raise Refused(link, b.halo, 0)
            st = Step(link, b.mask(), b.halo, block=b, need=(b.halo, 1))
        elif what == "block_stencil":
            b, r = R.block(link[3]), REACH[link[2]]
            if sharded and b.halo < r + 1:
                raise Refused(link, b.halo, r)
            st = Step(link, erode(b.mask(), r), b.halo - r if sharded else b.halo, src=b.mask(), block=b, need=(b.halo, r + 1))
        elif what == "blend":
            a, b = steps[link[2]], steps[link[3]]
            st = Step(link, a.mask & b.mask, min(a.halo, b.halo))
        elif what == "stencil":
            s, r = steps[link[3]], REACH[link[2]]
            if sharded and s.halo < r + 1:
                raise Refused(link, s.halo, r)
            st = Step(link, erode(s.mask, r), s.halo - r if sharded else s.halo, src=s.mask, need=(s.halo, r + 1))
        else:
            raise ValueError(link)
        steps[out] = st
    return steps


def telling_faces(R, st):
    """the (axis, side) of a sharded stencil link where the stored box ends on the volume's face while the source's valid
    box ends inside the volume: there "the stored box reaches the face" and "the source is valid up to the face" part"""
    if st.link[0] != "stencil":
        return []
    lo, hi = box_of(st.src)
    out = []
    for a in range(3):
        if R.stored_lo[a] == 0 and lo[a] > 0:
            out.append((a, 0))
        if R.stored_hi[a] == R.dims[a] and hi[a] < R.dims[a]:
            out.append((a, 1))
    return out


def between(R, st, face):
    """bool over the volume: the layers at `face` that the source holds valid and the result must not -- inside the source's
    valid box, between its end and the result's"""
    a, side = face
    (slo, shi), (lo, hi) = box_of(st.src), st.box
    blo, bhi = list(slo), list(shi)
    if side == 0:
        bhi[a] = lo[a]
    else:
        blo[a] = hi[a]
    return box_mask(R.dims, blo, bhi)


# ---- the chains

def chain_a(kind="merge"):
    return (("block", 1, 0, REACH[kind] + 1), ("stencil", 2, kind, 1))


def chain_c(kind):
    m = REACH[kind] + 1
    return (("block", 1, 0, m), ("block", 2, 1, m), ("blend", 3, 1, 2, 0.4), ("stencil", 4, kind, 3))


CHAIN_D = (("upload", 1, 0), ("stencil", 2, "merge", 1), ("stencil", 3, "derive", 2))
CHAIN_D2 = (("block", 1, 0, 4), ("stencil", 2, "merge", 1), ("stencil", 3, "derive", 2))
CHAIN_E = (("block_stencil", 1, "merge", 3), ("stencil", 2, "merge", 1))
CHAIN_F = (("upload", 1, 0), ("block", 2, 1, 2), ("blend", 3, 1, 2, 0.4), ("stencil", 4, "merge", 3))

# (id, dims, nranks, option halo, links).  The volumes are a few thousand voxels.  Bit 0 of a rank splits x, so a stored box
# that covers an axis AND a C that does not need option halo >= half the axis: 9..13 voxels with halo 4..6
CASES = (
    ("A-merge-9x11x13-r2-h4", (9, 11, 13), 2, 4, chain_a("merge")),          # rank 1: all of x stored (with a pad column), C from 2
    ("A-merge-10x11x13-r2-h5", (10, 11, 13), 2, 5, chain_a("merge")),        # both ranks; rank 0's upper face
    ("A-merge-9x9x9-r8-h4", (9, 9, 9), 8, 4, chain_a("merge")),              # every axis
    ("B-derive-11x9x13-r2-h5", (11, 9, 13), 2, 5, chain_a("derive")),
    ("B-derive-12x9x13-r2-h6", (12, 9, 13), 2, 6, chain_a("derive")),
    ("B-derive-13x13x13-r8-h6", (13, 13, 13), 8, 6, chain_a("derive")),
    ("B-derive-69x12x13-r4-h6", (69, 12, 13), 4, 6, chain_a("derive")),      # a stored box wider than a derive tile in x, an odd x
                                                                             # origin by the evening; the telling faces are y's
    ("C-derive-12x9x13-r2-h6", (12, 9, 13), 2, 6, chain_c("derive")),        # the playback flow
    ("C-merge-10x11x13-r2-h5", (10, 11, 13), 2, 5, chain_c("merge")),
    ("D-21x9x13-r2-h4", (21, 9, 13), 2, 4, CHAIN_D),                         # a second stencil from a source with a rim (uploaded: no telling face)
    ("D2-12x9x13-r2-h6", (12, 9, 13), 2, 6, CHAIN_D2),                       # ... from a block: telling faces at both stencils
    ("E-merge-10x11x13-r2-h5", (10, 11, 13), 2, 5, CHAIN_E),
    ("F-merge-9x11x13-r2-h4", (9, 11, 13), 2, 4, CHAIN_F),
)
CASE_IDS = [c[0] for c in CASES]
# An uploaded step is valid on all of the stored box, so every box a chain of stencils makes of it ends on the volume's face
# exactly where the stored box does: chain D cannot have a telling face (tests/test_step_chain_cpu.py asserts that it has none)
NO_TELLING_FACE = ("D-21x9x13-r2-h4",)
RINGS = S.RINGS

# chains the entries must refuse: (id, dims, nranks, option halo, links that pass, the refused link, (have, reach))
REFUSED = (
    ("derive-after-derive-h4", (21, 9, 13), 2, 4, (("upload", 1, 0), ("stencil", 2, "derive", 1)), ("stencil", 3, "derive", 2), (2, 2)),
    ("derive-after-a-block-of-2-ghosts", (12, 9, 13), 2, 6, (("block", 1, 0, 2),), ("stencil", 2, "derive", 1), (2, 2)),
    ("merge-after-a-block-of-1-ghost", (10, 11, 13), 2, 5, (("block", 1, 0, 1),), ("stencil", 2, "merge", 1), (1, 1)),
    ("derive-after-a-blend-with-a-block-of-2-ghosts", (12, 9, 13), 2, 6, (("upload", 1, 0), ("block", 2, 1, 2), ("blend", 3, 1, 2, 0.4)),
     ("stencil", 4, "derive", 3), (2, 2)),
)
REFUSED_IDS = [c[0] for c in REFUSED]


def ranks_of(case, ring):
    _, dims, nranks, halo, _ = CASES[case]
    return [Rank(dims, r, nranks, halo, ring) for r in range(nranks)]


def final(links):
    return links[-1][1]


def final_kind(links):
    return links[-1][2]


def stencil_links(links):
    return [l for l in links if l[0] == "stencil"]
