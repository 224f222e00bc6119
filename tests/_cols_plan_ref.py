"""The column-stream kernel's launch plan, restated as rules (the comments of smk_cols.h): the integer
arithmetic between a column size and what the kernel is launched with.  tests/test_cols_plan_cpu.py sweeps these rules and
proves what the kernel relies on; tests/test_gpu_cols_plans.py holds the plan the library reads back
(smk_get_stat "cols_plan_<field>") to them.

Not restated: how the planner picks the column size (cw x ch cells) -- the pixel footprint of a cell, float geometry.  cw and
ch are inputs here, taken from the read-back, and only their consequences are checked (columns(), jobs).

The rules:
  slice image   (cw + 1) x (ch + 1) voxels -- the bilinear halo -- of 8 (u8) or 16 (f32) bytes, rounded up to 16 bytes
  DMA           whole-KiB wave instructions of 64 lanes x 16 bytes: n_ch = ceil(slice_bytes / 1024); the last one has
                last_units = slice_bytes / 16 - 64 (n_ch - 1) lanes, 1..64; the counted wait takes an immediate < 64
  fixed LDS     4096 listed rays (8 bytes + 1 byte of entry position each), three tables of 256 + 4 words (slot addresses, two
                histograms), 32 control words, 64 bytes of slack, and the classification's tables (lds_tables)
  slots         what fits beside the fixed part in 160 KiB, at most 12, at most cols_ns where set; fewer than 3: refused
  maxfly        slices one loader keeps in flight: cols_fly or 2, at most (nslots - 2) / loaders (every loader's loads in
                flight and the two slices a sample reads must be in the ring together), at least 1; then lowered while
                n_ch * maxfly > 63
  wstep         slices a wave waits for beyond the two it reads: 0 below 5 slots, 1 below 7, else 2, or cols_wstep - 1; at
                most nslots - 2, because the load a consumer at position p waits for, p + 1 + wstep, is issued only while
                (p + 1 + wstep) - nslots < p
  takes         take_min = cols_take_min or 16 free lanes; take_wait = cols_take_wait - 1 or 3 turns
  cells         a box of 8-byte voxels has even x and y extents: where the volume's extent is odd it ends in a pad voxel.
                The pad is no cell of a column and, marching towards it, no slice position; marching away from it it is
                the first position (the kernel counts positions from the near end)
  chunks        the slice positions in equal chunks of at most cols_chunk (clamped to 4..256, default 128)
  keys          a segment key per column index along U, along V, and per chunk: ncu + ncv + nck - 2 of them, 64 to a mask
                word, at most 8 words"""

LDS_CAP = 160 * 1024
MAX_RAYS = 4096
MAX_CL = 256
MAX_SLOTS = 12
MAX_MASK_WORDS = 8
SHAPES = ((15, 1), (14, 2))       # (consumer waves, loader waves) of option cols_shape 1, 2 (0: the first)
FIELDS = ("cw ch ncu ncv slice_bytes n_ch last_units nslots maxfly wstep take_min take_wait cl nck nkeys mask_words "
          "shape perm dir").split()


class Refused(Exception):
    """the planner declines the frame; str(e) is its reason"""


def ceil_div(a, b):
    return -(-a // b)


def lds_tables(tf_mode, sv=0, sg=0, third_axis=False, nelts=3, s3v=0, s3g=0):
    """bytes of the classification's tables in LDS: the occupancy bitmap (a bit per texel, rows of whole words; only up to
    16 KiB, and with a 2-D table only on its alpha-first path) and the third axis's alpha row (2-D table, at most 3 channels
    and 1024 entries)"""
    ah = tf_mode == 1 and third_axis and nelts <= 3 and 2 <= sv <= 1024
    fast = tf_mode == 1 and (not third_axis or ah)
    occ = ceil_div(sv, 32) * sg * 4 if tf_mode == 1 else ceil_div(s3v, 32) * s3g * 4 if tf_mode == 2 else 0
    use_occ = 0 < occ <= 16384 and (fast or tf_mode == 2)
    return (sv * 4 if ah else 0) + (occ if use_occ else 0)


def fixed_lds(tables=0):
    return MAX_RAYS * (8 + 1) + 3 * (MAX_CL + 4) * 4 + 32 * 4 + 64 + tables


def slice_bytes(cw, ch, vb):
    return ceil_div((cw + 1) * (ch + 1) * vb, 16) * 16


def ring(cw, ch, vb, shape=0, ns=0, fly=0, wstep=0, take_min=0, take_wait=0, tables=0):
    """the ring's part of the plan; ns, fly, wstep, take_min, take_wait are the options cols_* (0: the planner decides)"""
    sb = slice_bytes(cw, ch, vb)
    n_ch = ceil_div(sb, 1024)
    p = dict(slice_bytes=sb, n_ch=n_ch, last_units=sb // 16 - 64 * (n_ch - 1))
    nslots = min((LDS_CAP - fixed_lds(tables)) // sb, MAX_SLOTS)
    if ns:
        nslots = min(nslots, ns)
    if nslots < 3:
        raise Refused("column slice does not fit LDS three times")
    loaders = SHAPES[shape][1]
    maxfly = max(1, min(fly if fly > 0 else 2, (nslots - 2) // loaders))
    while maxfly > 1 and n_ch * maxfly > 63:
        maxfly -= 1
    if n_ch > 63:
        raise Refused("column slice needs more than 63 DMA instructions")
    default = 0 if nslots < 5 else 1 if nslots < 7 else 2
    p.update(nslots=nslots, maxfly=maxfly, wstep=min(wstep - 1 if wstep else default, nslots - 2),
             take_min=take_min if take_min > 0 else 16, take_wait=take_wait - 1 if take_wait > 0 else 3)
    return p


def positions(ns, padded=False, direction=1):
    """slice positions of a volume of ns slices along S; padded: its box of 8-byte voxels has a pad slice beyond the last"""
    return ns - 1 + (1 if padded and direction < 0 else 0)


def chunks(npos, chunk=0):
    """(cl, nck): positions per chunk and chunks of npos slice positions under option cols_chunk"""
    most = max(min(chunk, MAX_CL) if chunk else 128, 4)
    cl = ceil_div(npos, ceil_div(npos, most))
    return cl, ceil_div(npos, cl)


def columns(cells, c):
    """columns of c cells over `cells` cells (the last one ragged where c does not divide them)"""
    return ceil_div(cells, c)


def keys(ncu, ncv, nck):
    nkeys = ncu + ncv + nck - 2
    words = ceil_div(nkeys, 64)
    if words > MAX_MASK_WORDS:
        raise Refused("more than 512 segment keys")
    return nkeys, words


def plan(cw, ch, nu, nv, npos, vb, shape=0, chunk=0, tables=0, **knobs):
    """every field of the read-back that follows from the column size: nu x nv voxels of the volume (of a shard: of its
    box) along U and V, npos slice positions"""
    p = dict(cw=cw, ch=ch, ncu=columns(nu - 1, cw), ncv=columns(nv - 1, ch), shape=shape)
    p.update(ring(cw, ch, vb, shape=shape, tables=tables, **knobs))
    p["cl"], p["nck"] = chunks(npos, chunk)
    p["nkeys"], p["mask_words"] = keys(p["ncu"], p["ncv"], p["nck"])
    p["jobs"] = p["ncu"] * p["ncv"] * p["nck"]
    return p


def entry_positions(npos, chunk=0):
    """the largest entry position a job stores (a byte per listed ray): a chunk's positions are 0 .. cl - 1"""
    cl, nck = chunks(npos, chunk)
    return cl - 1


def n_ch_class(n):
    return "1" if n == 1 else "2..4" if n <= 4 else "5" if n == 5 else "6..8" if n <= 8 else "9" if n == 9 else "31" if n == 31 else "10+"


def last_class(u):
    return "1" if u == 1 else "64" if u == 64 else "2..63"


def nslots_class(n):
    return "3" if n == 3 else "4" if n == 4 else "5..6" if n <= 6 else "7..11" if n <= 11 else "12"
