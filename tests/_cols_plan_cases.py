"""The cases of the column-stream kernel's plan sweep (tests/test_gpu_cols_plans.py), their data, the classes a plan falls
into and the coverage tally.  Modelled on tests/_slab_plan_cases.py.

Dialling.  A volume is (Nu, Nv, Ns) voxels along the kernel's U, V and its marching axis S.  Under a window of 20 x 20 pixels
fewer rays cross the whole face than a workgroup has lanes, and one column has the least halo: the planner takes the face as
ONE column, cw = Nu - 1, ch = Nv - 1, and the slice image is exactly Nu x Nv voxels -- the voxel counts dial the DMA class
(n_ch, the last instruction's lanes) directly, and with it the slots that fit LDS.  A u8 volume of 2 Nu x Nv voxels has the
image bytes of the f32 volume of Nu x Nv.  Larger windows, or a small cols_fill, give several, ragged columns; their sizes
are the planner's float geometry and are taken from the read-back.

Every base case runs as three variants -- a, b, c: S = z, y, x; a and b in opposite marching directions; workgroup shapes
1, 2 and voxel types f32, u8 alternating -- so that each class is reached on every principal axis, in both directions, at
both shapes and for both voxel types without crossing them.  `want` holds what the base was dialled to (worked out by hand
from the voxel counts; tests/test_cols_plan_cpu.py holds it to the rules of tests/_cols_plan_ref.py, and the sweep holds the
read-back to both).

Data.  Noise seeded by the case's name, so a 16-byte unit fetched from a wrong place holds other numbers.  The table is
random colours with alpha bytes in [a, 2a], a sized to the samples that see material so that no ray saturates (the kernel's
sample count then equals the checker's).  `ends` cases -- long volumes, many chunks, many keys -- have material only in a thin
slab at either end of S: between them the value channel sits in a band the table leaves clear, so a ray has a handful of
non-empty segments whatever the number of jobs it crosses (the 2e-5 bound against the gather kernel rests on that), while
their keys lie in the first and the last mask word."""
import numpy as np

import _cols_plan_ref as ref
import oracle as O
from _slab_plan_cases import POSES, _seed, model_dims

TABLE = 256                                  # the (v, g) table is TABLE x TABLE texels
TABLES_LDS = ref.lds_tables(1, TABLE, TABLE)  # its occupancy bitmap in LDS
CLEAR_BELOW = 44                             # `ends`: table columns (values) below this are clear
KNOBS = ("cols_shape", "cols_ns", "cols_chunk", "cols_wstep", "cols_fill", "cols_take_min", "cols_take_wait", "cols_fly")
_REF_KNOB = {"cols_ns": "ns", "cols_fly": "fly", "cols_wstep": "wstep", "cols_take_min": "take_min", "cols_take_wait": "take_wait"}


def base(name, nu, nv, ns, cls, want=None, opts=None, size=(20, 20), one=True, ends=0.0, steps=None, fill=0.8, depth=0.4,
         refused=None, shape=0):
    """shape: the workgroup shape of every variant (0: they alternate)"""
    return dict(name=name, nu=nu, nv=nv, ns=ns, cls=cls.split(", "), want=want or {}, opts=opts or {}, size=size, one=one, ends=ends,
                steps=steps, fill=fill, depth=depth, refused=refused, shape=shape)


# ---- DMA width: Nu x Nv f32 voxels = Nu Nv 16-byte units (64 to an instruction); every slice image beside 48368 fixed
# bytes in 163840: slots = min(115472 // bytes, 12)
_DMA = [
    base("dma1-full", 8, 8, 7, "n_ch 1, last 64, nslots 12, maxfly 2, wstep 2, take_min 16, take_wait 3, one chunk, one column, mask_words 1",
         dict(slice_bytes=1024, n_ch=1, last_units=64, nslots=12, maxfly=2, wstep=2, take_min=16, take_wait=3, cl=6, nck=1, nkeys=1)),
    base("dma2-last1", 5, 13, 9, "n_ch 2..4, last 1", dict(slice_bytes=1040, n_ch=2, last_units=1, nslots=12)),
    base("dma4-full", 16, 16, 8, "n_ch 2..4, last 64", dict(slice_bytes=4096, n_ch=4, last_units=64, nslots=12)),
    base("dma5-full", 16, 20, 10, "n_ch 5, last 64", dict(slice_bytes=5120, n_ch=5, last_units=64, nslots=12)),
    base("dma7", 21, 19, 8, "n_ch 6..8, last 2..63", dict(slice_bytes=6384, n_ch=7, last_units=15, nslots=12)),
    base("dma9-last1", 19, 27, 9, "n_ch 9, last 1", dict(slice_bytes=8208, n_ch=9, last_units=1, nslots=12)),
    # 720 units: 12 instructions; 10 slots; eight slices in flight asked: (10 - 2) / 1 = 8 allowed by the slots, 63 // 12 = 5
    # by the counted wait (which is then asked for 48) -- at shape 1: the class is unreachable with two loaders, see the tally
    base("dma12-fly8", 24, 30, 12, "n_ch 10+, nslots 7..11, maxfly 3+, maxfly lowered by n_ch",
         dict(slice_bytes=11520, n_ch=12, last_units=16, nslots=10, maxfly=5, wstep=2), opts={"cols_fly": 8}, shape=1),
    base("dma12", 24, 30, 12, "n_ch 10+, nslots 7..11", dict(slice_bytes=11520, n_ch=12, last_units=16, nslots=10, wstep=2)),
    base("dma18-ring6", 32, 36, 7, "n_ch 10+, nslots 5..6, wstep 1", dict(slice_bytes=18432, n_ch=18, last_units=64, nslots=6, wstep=1)),
    # (6 - 2) / 1 = 4 by the slots, 63 // 18 = 3 by the wait
    base("dma18-fly8", 32, 36, 7, "maxfly 3+, maxfly lowered by n_ch", dict(n_ch=18, nslots=6, maxfly=3), opts={"cols_fly": 8}, shape=1),
    base("dma24-ring4", 38, 40, 6, "n_ch 10+, nslots 4, wstep 0", dict(slice_bytes=24320, n_ch=24, last_units=48, nslots=4, wstep=0),
         opts={"cols_ns": 4}),
    # the largest slice: 1980 units, 62 instructions with two slices in flight (the planner's limit for a column); three slots
    base("dma31-ring3", 44, 45, 6, "n_ch 31, nslots 3, maxfly 1, wstep 0", dict(slice_bytes=31680, n_ch=31, last_units=60, nslots=3, maxfly=1, wstep=0),
         opts={"cols_ns": 3}),
]
# ---- ring knobs on small slices (12 slots unless capped), more slices than slots
_RING = [
    base("fly3", 12, 10, 30, "maxfly 3+", dict(n_ch=2, last_units=56, nslots=12, maxfly=3), opts={"cols_fly": 3}),
    base("fly12", 8, 8, 30, "maxfly 3+, maxfly lowered by slots", dict(n_ch=1, nslots=12), opts={"cols_fly": 12}),
    base("fly1", 8, 8, 20, "maxfly 1", dict(maxfly=1, nslots=12), opts={"cols_fly": 1}),
    base("wstep0", 8, 8, 20, "wstep 0", dict(wstep=0, nslots=12), opts={"cols_wstep": 1}),
    base("wstep1", 8, 8, 20, "wstep 1", dict(wstep=1, nslots=12), opts={"cols_wstep": 2}),
    base("wstep6", 8, 8, 20, "wstep 3+", dict(wstep=6, nslots=12), opts={"cols_wstep": 7}),
    # a band wait the ring cannot hold: asked 3 with 3 slots, asked 6 with 4 -- clamped to nslots - 2
    base("wstep-clamp-ns3", 8, 8, 20, "wstep clamped, wstep 1, nslots 3, maxfly 1", dict(wstep=1, nslots=3, maxfly=1),
         opts={"cols_wstep": 4, "cols_ns": 3}),
    base("wstep-clamp-ns4", 10, 8, 20, "wstep clamped, wstep 2, nslots 4", dict(wstep=2, nslots=4), opts={"cols_wstep": 7, "cols_ns": 4}),
    base("ns5", 8, 8, 20, "nslots 5..6, wstep 1", dict(nslots=5, wstep=1), opts={"cols_ns": 5}),
    base("ns7", 10, 8, 20, "nslots 7..11, wstep 2", dict(nslots=7, wstep=2, maxfly=2), opts={"cols_ns": 7}),
    base("take1", 12, 10, 20, "take_min 1, take_wait 0", dict(take_min=1, take_wait=0), opts={"cols_take_min": 1, "cols_take_wait": 1}),
    base("take64", 12, 10, 20, "take_min 64, take_wait 49", dict(take_min=64, take_wait=49), opts={"cols_take_min": 64, "cols_take_wait": 50}),
]
# ---- chunks: the Ns - 1 positions in equal chunks
_CHUNK = [
    base("chunk4-short-last", 8, 8, 11, "cl 4, short last chunk", dict(cl=4, nck=3, nkeys=3), opts={"cols_chunk": 4}),
    base("cl256", 8, 8, 257, "cl 256, one chunk", dict(cl=256, nck=1), opts={"cols_chunk": 256}, ends=0.04, steps=340),
    base("cl256-two", 8, 8, 513, "cl 256", dict(cl=256, nck=2), opts={"cols_chunk": 256}, ends=0.03, steps=670),
    base("two-slices", 12, 10, 2, "two slices, one chunk", dict(cl=1, nck=1)),
    base("chunks-default", 8, 8, 300, "short last chunk", dict(cl=100, nck=3), ends=0.04, steps=200),
]
# ---- several columns (their sizes are the planner's; the sweep takes them from the read-back)
_COLS = [
    base("cols-window96", 42, 30, 12, "several columns", size=(96, 96), fill=0.9, one=False),
    base("cols-window-odd", 38, 32, 10, "several columns", size=(91, 67), fill=0.9, one=False),
    base("cols-fill10", 24, 18, 9, "several columns", opts={"cols_fill": 10}, one=False),
]
# ---- segment keys: ncu + ncv + nck - 2, 64 to a mask word
_KEYS = [
    base("keys70", 8, 8, 281, "mask_words 2, cl 4", dict(cl=4, nck=70, nkeys=70, mask_words=2), opts={"cols_chunk": 4}, ends=0.05, steps=120),
    # 480 chunks; the 48 x 48 window holds more rays than lanes, so the 7 x 7 (u8: 15 x 7) cells split into columns: 480 to
    # 500 keys, the eighth mask word whatever the split
    base("keys480", 8, 8, 1921, "mask_words 8, cl 4, several columns", dict(cl=4, nck=480, mask_words=8), opts={"cols_chunk": 4}, ends=0.05,
         steps=96, size=(48, 48), fill=0.9, one=False),
]
BASES = _DMA + _RING + _CHUNK + _COLS + _KEYS
# the refusal just beyond the last mask word: 515 chunks
REFUSED_KEYS = base("keys515", 8, 8, 2061, "", opts={"cols_chunk": 4}, ends=0.05, steps=96, size=(48, 48), fill=0.9, one=False,
                    refused="more than 512 segment keys")

_VARIANTS = (("a", ("z+", "z-")), ("b", ("y-", "y+")), ("c", ("x+", "x-")))


def padded_s(c):
    """a box of 8-byte voxels has even x and y extents: an odd count of slices along S = x or y ends in a pad slice"""
    return (not c["f32"]) and c["pose"][0] in "xy" and c["ns"] % 2 == 1


def _finish(c):
    if c["f32"] is False:
        c["nu"] = 2 * c["nu"]                   # the f32 image's bytes
    c["dims"] = model_dims(c["pose"], c["nu"], c["nv"], c["ns"])
    if c["steps"] is None:
        c["steps"] = int(min(max(1.3 * c["ns"] + 3, 8), 160))
    return c


def _variants(k, b):
    """the three variants of base k: u8 and f32 alternate, but a u8 variant whose box would be padded along S (the chunk
    classes then depend on the marching direction: the pad cases below) is f32 instead, and one variant is u8 in any case"""
    poses = [p[k % 2] for _, p in _VARIANTS]
    f32 = [(j + k) % 2 == 0 or (poses[j][0] in "xy" and b["ns"] % 2 == 1) for j in range(3)]
    if all(f32):
        f32[0] = False                          # (S = z is never padded)
    return [_finish(dict(b, name="%s-%s" % (b["name"], tag), base=b["name"], pose=poses[j], f32=f32[j],
                         shape=b["shape"] or 1 + (j + k // 2) % 2)) for j, (tag, _) in enumerate(_VARIANTS)]


def _explicit(b, variants):
    """a base whose variants are listed: (pose, f32, shape)"""
    return [_finish(dict(b, name="%s-%s" % (b["name"], "abcdef"[j]), base=b["name"], pose=pose, f32=f32, shape=shape))
            for j, (pose, f32, shape) in enumerate(variants)]


CASES = [c for k, b in enumerate(BASES) for c in _variants(k, b)]
# ---- 8-byte voxels only
# an odd count of them: 9 x 11 = 99 voxels are 792 bytes, rounded up to 800 = 50 units (the stored box is 10 x 12: the pad is no cell)
CASES += _explicit(base("u8-odd", 9, 11, 8, "n_ch 1, last 2..63, u8 image of an odd voxel count", dict(slice_bytes=800, n_ch=1, last_units=50)),
                   (("z-", None, 2), ("y+", None, 1), ("x-", None, 2)))
# 65 units of them: 10 x 13 = 130 voxels, a last instruction of one lane
CASES += _explicit(base("u8-last1", 10, 13, 10, "n_ch 2..4, last 1", dict(slice_bytes=1040, n_ch=2, last_units=1)),
                   (("x+", None, 1), ("z+", None, 2), ("y-", None, 1)))
# a pad slice along S: 41 slices in a box of 42.  Marching towards the pad there are 40 positions in 10 chunks of 4 (41 in 11
# would make the pad a chunk of its own, whose job takes the volume's last half voxel a second time); marching away from it
# the pad is position 0 of 41, in 11 chunks
CASES += _explicit(base("pad-chunk", 16, 8, 41, "cl 4", dict(cl=4), opts={"cols_chunk": 4}),
                   (("y+", None, 1), ("y-", None, 2), ("x+", None, 2), ("x-", None, 1)))
# a pad cell along U or V: 33 voxels in a box of 34, 32 cells in columns (33 cells in columns of 2, 4, 8, 16 or 32 would make
# the pad a column of its own: the same double take, across the whole face)
CASES += _explicit(base("pad-columns-u", 33, 16, 10, "several columns", size=(64, 64), fill=0.9, one=False),
                   (("z+", None, 1), ("y-", None, 2), ("x+", None, 1)))
CASES += _explicit(base("pad-columns-v", 16, 33, 10, "several columns", size=(64, 64), fill=0.9, one=False),
                   (("z-", None, 2),))
for _c in CASES:
    if _c["f32"] is None:                       # (_explicit: u8 without the doubling of nu)
        _c["f32"] = False
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
REFUSED_CASE = _variants(1, REFUSED_KEYS)[0]


def ref_knobs(c):
    """the case's options as tests/_cols_plan_ref.py names them"""
    return {_REF_KNOB[k]: v for k, v in c["opts"].items() if k in _REF_KNOB}


def expected_plan(c, cw=None, ch=None, direction=1):
    """the rules' plan of the case; one-column cases need no read-back (but for the marching direction where the box is
    padded along S)"""
    if cw is None:
        assert c["one"]
        cw, ch = c["nu"] - 1, c["nv"] - 1
    return ref.plan(cw, ch, c["nu"], c["nv"], ref.positions(c["ns"], padded_s(c), direction), 16 if c["f32"] else 8, shape=c["shape"] - 1,
                    chunk=c["opts"].get("cols_chunk", 0), tables=TABLES_LDS, **ref_knobs(c))


# ------------------------------------------------------------------------------------------------ classes
def classes_of(c, p):
    """the classes a plan (read back, or the rules') of the case falls into"""
    nl = ref.SHAPES[p["shape"]][1]
    out = {"n_ch " + ref.n_ch_class(p["n_ch"]), "last " + ref.last_class(p["last_units"]), "nslots " + ref.nslots_class(p["nslots"])}
    out.add("maxfly %s" % ("3+" if p["maxfly"] >= 3 else p["maxfly"]))
    fly = c["opts"].get("cols_fly", 0)
    by_slots = max(1, (p["nslots"] - 2) // nl)
    if fly > p["maxfly"]:
        if p["maxfly"] == by_slots and p["n_ch"] * by_slots <= 63:
            out.add("maxfly lowered by slots")
        elif p["maxfly"] == 63 // p["n_ch"] < by_slots:
            out.add("maxfly lowered by n_ch")
    out.add("wstep %s" % ("3+" if p["wstep"] >= 3 else p["wstep"]))
    asked = c["opts"].get("cols_wstep", 0) - 1
    if asked > p["nslots"] - 2 and p["wstep"] == p["nslots"] - 2:
        out.add("wstep clamped")
    out.add("take_min %d" % p["take_min"])
    out.add("take_wait %d" % p["take_wait"])
    if p["nck"] == 1:
        out.add("one chunk")
    if p["cl"] in (4, 256):
        out.add("cl %d" % p["cl"])
    direction = p.get("dir", 1)
    if ref.positions(c["ns"], padded_s(c), direction) % p["cl"]:
        out.add("short last chunk")
    if padded_s(c):
        out.add("pad slice ahead of the march" if direction > 0 else "pad slice behind the march")
    if not c["f32"]:
        if c["nu"] % 2 and p["ncu"] > 1:
            out.add("pad cell beyond the last column along U")
        if c["nv"] % 2 and c["pose"][0] == "z" and p["ncv"] > 1:
            out.add("pad cell beyond the last column along V")
        if (p["cw"] + 1) * (p["ch"] + 1) % 2:
            out.add("u8 image of an odd voxel count")
    if c["ns"] == 2:
        out.add("two slices")
    if p["ncu"] * p["ncv"] == 1:
        out.add("one column")
    else:
        out.add("several columns")
        if p["ncu"] > 1 and p["ncu"] * p["cw"] > c["nu"] - 1:
            out.add("ragged last column along U")
        if p["ncv"] > 1 and p["ncv"] * p["ch"] > c["nv"] - 1:
            out.add("ragged last column along V")
        if p["cw"] != p["ch"]:
            out.add("several columns, cw != ch")
    out.add("mask_words %d" % p["mask_words"])
    return out


# every class the sweep must reach (the issue's list)
CLASSES = (["n_ch " + k for k in ("1", "2..4", "5", "6..8", "9", "10+", "31")] + ["last " + k for k in ("1", "2..63", "64")] +
           ["nslots " + k for k in ("3", "4", "5..6", "7..11", "12")] +
           ["maxfly 1", "maxfly 2", "maxfly 3+", "maxfly lowered by n_ch", "maxfly lowered by slots"] +
           ["wstep 0", "wstep 1", "wstep 2", "wstep clamped"] + ["take_min 1", "take_min 16", "take_min 64"] +
           ["take_wait 0", "take_wait 3", "take_wait 49"] + ["one chunk", "cl 4", "short last chunk", "cl 256", "two slices"] +
           ["one column", "several columns", "ragged last column along U", "ragged last column along V", "several columns, cw != ch"] +
           ["mask_words 1", "mask_words 2", "mask_words 8"])
# (class, axis value) pairs no plan reaches.  With two loaders maxfly <= (nslots - 2) / 2 and the ring fits 115472 bytes beside
# the fixed LDS, nslots * (1024 n_ch - 1008) <= 115472: n_ch * maxfly <= n_ch (nslots - 2) / 2 < 63 for every n_ch and nslots
# (tests/test_cols_plan_cpu.py sweeps it), so the n_ch * maxfly <= 63 rule never lowers a request at shape 2.
UNREACHABLE = {("maxfly lowered by n_ch", "shape", 1)}
# classes of 8-byte voxels alone: reached at all (a pad exists along x and y only)
U8_CLASSES = ["u8 image of an odd voxel count", "pad slice ahead of the march", "pad slice behind the march",
              "pad cell beyond the last column along U", "pad cell beyond the last column along V"]
AXES = (("shape", (0, 1)), ("f32", (True, False)), ("dir", (1, -1)), ("perm", (0, 1, 2)))


def tally(records):
    """records: [(case, plan dict)].  Returns (rows, missing): a row per class with the cases that reach it and what they cover,
    and the (class, axis, value) the issue asks for that no record reaches"""
    rows, missing = [], []
    recs = [(c, dict(p, f32=c["f32"]), classes_of(c, p)) for c, p in records]
    for cls in CLASSES:
        mine = [(c, p) for c, p, k in recs if cls in k]
        lack = []
        for axis, values in AXES:
            for v in values:
                if (cls, axis, v) in UNREACHABLE:
                    continue
                if not any(p[axis] == v for _, p in mine):
                    lack.append("%s %s" % (axis, v))
                    missing.append("%s at %s %s" % (cls, axis, v))
        rows.append("| %s | %d | %s | %s |" % (cls, len(mine), ", ".join(sorted({c["base"] for c, _ in mine})) or "-",
                                                "every shape, type, direction and axis" if not lack else "MISSING " + ", ".join(lack)))
    for cls in U8_CLASSES:
        mine = sorted({c["base"] for c, p, k in recs if cls in k})
        rows.append("| %s | %d | %s | %s |" % (cls, len(mine), ", ".join(mine) or "-", "reached" if mine else "MISSING"))
        if not mine:
            missing.append(cls)
    return rows, missing


# ------------------------------------------------------------------------------------------------ data
def _s_axis(c):
    return {"z": 0, "y": 1, "x": 2}[c["pose"][0]]     # of the [nz][ny][nx] arrays


def end_slabs(c):
    """(first, last) slab thickness in slices of an `ends` case"""
    e = max(2, int(round(c["ends"] * c["ns"])))
    return e, e


def noise_volume(c, keep=(True, True)):
    """(u8 VGH, f32 VGH) of the case: [nz][ny][nx][3]; `keep`: which end slab of an `ends` case holds material"""
    nx, ny, nz = c["dims"]
    rng = np.random.default_rng(_seed(c["name"]))
    v8 = rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
    vf = rng.random((nz, ny, nx, 3), dtype=np.float32)
    if c["ends"]:
        # material: values well above the clear band; between the slabs a value inside it
        v8[..., 0] = 64 + v8[..., 0] % 192
        vf[..., 0] = np.float32(0.25) + vf[..., 0] * np.float32(0.75)
        e0, e1 = end_slabs(c)
        lo, hi = (e0 if keep[0] else 0), (c["ns"] - e1 if keep[1] else c["ns"])
        sl = [slice(None)] * 4
        sl[_s_axis(c)] = slice(lo, hi)
        sl[3] = 0
        v8[tuple(sl)] = 10
        vf[tuple(sl)] = np.float32(10.0 / 255.0)
    return v8, vf


def material_samples(c):
    """samples of a ray that see material, roughly: all of them, or those inside the two end slabs"""
    return c["steps"] * (sum(end_slabs(c)) / c["ns"] if c["ends"] else 1.0)


def table_alpha(c):
    """alpha bytes are drawn from [a, 2a]: at most 2.4 optical depths over the samples that see material, so no ray's
    alpha rounds to 1.0f (that takes 16.6) and early termination never drops a sample"""
    return int(min(max(round(255.0 * 1.2 / max(material_samples(c), 1.0)), 2), 40))


def table2d(c):
    rng = np.random.default_rng(_seed(c["name"]) ^ 0x7ab1e)
    a = table_alpha(c)
    t = rng.integers(0, 256, (TABLE, TABLE, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(a, 2 * a + 1, (TABLE, TABLE), dtype=np.uint8)
    if c["ends"]:
        t[:, :CLEAR_BELOW, 3] = 0
    return t


def build_scene(c, keep=(True, True)):
    v8, vf = noise_volume(c, keep)
    ax = {"z": 2, "y": 1, "x": 0}[c["pose"][0]]
    fsize = [c["fill"]] * 3
    fsize[ax] = c["depth"]
    sc = O.Scene(vf if c["f32"] else v8, fsize=tuple(fsize), grad=O.normals_vgh(v8))
    sc.tf_mode = 1
    sc.tf_vg = table2d(c)
    sc.width, sc.height = c["size"]
    sc.steps = c["steps"]
    sc.xform = O.rotation(*POSES[c["pose"]])
    sc.shade_mode = 1
    return sc
