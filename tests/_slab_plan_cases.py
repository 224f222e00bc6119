"""The cases of the slice-ring kernel's plan sweep (tests/test_gpu_slab_plans.py), their data, and the coverage tally.

Data.  Every voxel of every channel is noise seeded by the case's name alone -- u8 VGH bytes and f32 VGH floats drawn
independently -- so a 16-byte unit fetched from a wrong place holds other numbers than the right one.  Two tables:
"dense" (random colours, every texel with a small non-zero alpha drawn from [a, 2a], a sized to the case's plane count so
that no ray saturates and the loaders stream every slice) and "sparse" (the same with bands of clear texels, so that the
occupancy bits, the bitmap in LDS and the brick flags engage; `hole` confines a third of the slices to the clear band, so
that whole layers of bricks come out empty).  tests/test_slab_plan_cases_cpu.py holds the generator to this with the
checker alone.

Cases.  A volume is (Nu, Nv, Ns) voxels along the kernel's window axes U, V and its marching axis S; the pose names S and
the direction.  The world size of the box is chosen per case (`fill` of the view across, `depth` along S) and has nothing to
do with the voxel counts, so a 64 x 2 x 6 slab fills the image like a cube does.  A frame of ONE tile that sees the whole
volume gets its window from the stored extent: wu = Nu 16-byte units (f32; u8 packs two voxels per unit) and wv = Nv rows --
the voxel counts dial the pitch class exactly.  PLANS records, per case, the plan the planner gave it when the case was
dialled; the sweep asserts it on the read-back."""
import zlib

import numpy as np

import oracle as O

# S axis and direction; a few degrees off the axis so that no ray coefficient is exactly zero
POSES = {"z+": ((0.3, 1, 0.2), 3), "z-": ((0.1, 1, 0.05), 177),
         "y+": ((1, 0.05, 0.03), 87), "y-": ((1, -0.03, 0.05), -93),
         "x+": ((0.03, 1, 0.05), 87), "x-": ((0.05, 1, -0.03), -93)}
# workgroup shapes of option "tile": id -> (tw, th, big)
TILES = {2: (24, 32, True), 4: (32, 24, True), 5: (32, 16, False), 7: (16, 32, False), 12: (48, 16, True), 13: (16, 48, True),
         19: (48, 16, True), 20: (40, 16, False), 21: (16, 40, False)}
PLAN_FIELDS = ("tw th nw nl wu wv wp per rpg groups chunks mych nslots maxfly wstep pmask mask_need use_occ use_ah fast_tf "
               "bricks perm dir lds_bytes slices_max").split()


def model_dims(pose, nu, nv, ns):
    """(nx, ny, nz) of a volume of nu x nv x ns voxels along U, V, S (SlabParams: S = z: U = x, V = y; S = y: U = x, V = z;
    S = x: U = y, V = z)"""
    return {"z": (nu, nv, ns), "y": (nu, ns, nv), "x": (ns, nu, nv)}[pose[0]]


def case(name, pose, nu, nv, ns, f32=True, table="dense", tile=0, size=None, **kw):
    c = dict(name=name, pose=pose, nu=nu, nv=nv, ns=ns, f32=f32, table=table, tile=tile, fill=0.8, depth=0.4, opts={}, blend=0,
             feature=None, hole=False, tsize=256, shade=1, steps=None, frustum=1.0)
    c.update(kw)
    if size is None:
        size = TILES[tile][:2] if tile else (16, 16)      # one tile, whatever shape the planner takes
    c["size"] = size
    c["dims"] = model_dims(pose, nu, nv, ns)
    if c["steps"] is None:
        c["steps"] = int(min(max(1.3 * ns + 3, 8), 160))
    return c


# ---- the pitch family: per class (wp: rpg) a window with wu == wp in ONE row group and one with wu < wp in three or more,
# the last of them ragged where rpg > 1; f32 for every class, u8 too where wp <= 32 (a u8 row of 66 voxels is 33 units).
# Where the pitch is a multiple of 4 only (4, 12, 20, 28) the rows are chosen so that it takes fewer chunks than the next
# multiple of 8 (tests/_slab_plan_ref.py).
_PITCH = [(4, (4, 16), (3, 40)), (8, (8, 8), (7, 20)), (12, (12, 16), (11, 40)), (16, (16, 4), (15, 11)), (20, (20, 16), (19, 44)),
          (24, (24, 8), (23, 20)), (28, (28, 16), (27, 44)), (32, (32, 2), (31, 5)), (40, (40, 8), (39, 20)), (48, (48, 4), (47, 11)),
          (56, (56, 8), (55, 20)), (64, (64, 3), (63, 5))]
_TILE_TURN = [5, 2, 20, 4, 7, 12, 21, 13, 0, 19]
_TABLE_TURN = ["dense", "sparse", "dense"]


def _pitch_cases():
    out, k = [], 0
    poses = sorted(POSES)
    for wp, one, three in _PITCH:
        for f32 in (True, False):
            if not f32 and wp > 32:
                continue
            for tag, (wu, wv) in (("g1", one), ("g3", three)):
                tile = _TILE_TURN[k % len(_TILE_TURN)]
                out.append(case("p%d-%s-%s" % (wp, "f32" if f32 else "u8", tag), poses[k % 6], wu if f32 else 2 * wu, wv,
                                6 + 5 * (k % 7), f32=f32, table=_TABLE_TURN[k % 3], tile=tile, want=dict(wp=wp, wu=wu, wv=wv)))
                k += 1
    return out


def _ring_cases():
    c = []
    # a ring of 24 slots (3 chunks a slice) under a volume of 24 slices: slices == slots; no per-slice extents
    c.append(case("ring24-eq", "z+", 12, 16, 24, tile=5))
    # the same ring capped at 3 slots (slab_ns) under more slices than slots
    c.append(case("ring3-forced", "y-", 12, 16, 40, tile=7, opts={"slab_ns": 3}))
    # 49 chunks a slice: three slots are all one CU's LDS holds (natural nslots == 3), mych = 49 >= 32 binds maxfly at 2
    # whatever slab_fly asks; on a big workgroup the same window is the largest mych its LDS allows (28)
    c.append(case("ring3-natural-small", "z-", 56, 56, 9, tile=20, tsize=32, opts={"slab_fly": 3}))
    c.append(case("mych-max-big", "z+", 56, 56, 9, tile=4, tsize=32, table="sparse"))
    # 52 chunks a slice on a small workgroup: the largest mych its LDS allows
    c.append(case("mych-max-small", "y+", 64, 52, 7, tile=20, tsize=32))
    # long sticks: more than 64 and more than 128 slices at per 3 and per 5 (slice-table blocks, ring wrap), a ring
    # between 3 and 24 slots, a deep band (fewer planes than slices: wstep >= 2)
    c.append(case("stick-100", "x+", 24, 8, 100, tile=7, table="sparse", hole=True))
    c.append(case("stick-200", "z-", 20, 16, 200, tile=5, steps=60))
    c.append(case("stick-200-u8", "y+", 40, 16, 150, f32=False, tile=4, table="sparse", hole=True))
    c.append(case("stick-fly3", "x-", 20, 16, 70, tile=21, opts={"slab_fly": 3}))
    c.append(case("stick-T1", "z+", 24, 8, 70, tile=2, opts={"slab_T": 1}))
    c.append(case("stick-T2", "y-", 24, 8, 70, tile=12, opts={"slab_T": 2}))
    c.append(case("stick-T3", "z-", 24, 8, 70, tile=20, opts={"slab_T": 3}, table="sparse"))
    return c


def _flag_cases():
    c = []
    c.append(case("third-axis", "z+", 20, 16, 12, tile=5, table="dense_h"))              # cfg 4: use_ah
    c.append(case("third-axis-u8", "x+", 40, 44, 12, f32=False, tile=4, table="sparse_h"))
    # (the planner drops the flags where no brick comes out empty -- here; stick-100 and stick-200-u8 keep them)
    c.append(case("bricks-off", "y+", 24, 20, 30, tile=20, table="sparse", hole=True, opts={"bricks": 0}))
    c.append(case("bricks-on", "y+", 24, 20, 30, tile=20, table="sparse", hole=True))
    c.append(case("big-table", "z-", 24, 20, 10, tile=5, table="sparse", tsize=(512, 256)))   # occupancy bitmap over 8 KiB: not in LDS
    c.append(case("tf3d-occ", "x-", 24, 20, 10, tile=7, table="dense3d", shade=0))
    c.append(case("tf3d-noocc", "z+", 12, 16, 10, tile=5, table="dense3d"))                    # 3 chunks: no per-slice extents, no bitmap
    c.append(case("tf3d-u8", "y-", 40, 16, 10, f32=False, tile=13, table="dense3d"))
    return c


def _geometry_cases():
    c = []
    c.append(case("two-slices", "z+", 20, 16, 2, tile=5))
    c.append(case("three-slices", "y-", 20, 16, 3, tile=7))
    c.append(case("three-slices-u8", "x+", 24, 12, 3, f32=False, tile=0))
    # several tiles: windows narrower than the box, the border tiles' windows clamp at both of its faces
    c.append(case("tiles-2x3", "z+", 66, 60, 20, tile=5, size=(64, 48), fill=0.9))
    c.append(case("tiles-auto-odd", "y+", 50, 45, 24, tile=0, size=(59, 37), fill=0.9, table="sparse"))
    c.append(case("tiles-big-u8", "x-", 66, 66, 16, f32=False, tile=2, size=(47, 63), fill=0.95))
    c.append(case("tiles-big-f32", "z-", 66, 66, 16, tile=4, size=(63, 47), fill=0.95, table="sparse"))
    # a close-up under a wide frustum: the corner rays drift more than 2 voxels per slice (under the planner's limit of 3)
    c.append(case("closeup", "z+", 40, 40, 4, tile=5, size=(64, 48), fill=1.6, depth=1.2, frustum=4.0))
    return c


def _instance_cases():
    c = []
    c.append(case("shadows", "z+", 20, 16, 12, tile=5, feature="shadows"))
    c.append(case("occluded", "y+", 24, 20, 12, tile=7, feature="occluded"))
    c.append(case("split3", "x+", 28, 16, 40, tile=20, opts={"slab_split": 3}))
    c.append(case("first-hit-depth", "z-", 40, 20, 12, tile=4, table="sparse", feature="depth"))
    c.append(case("back-to-front", "y-", 20, 16, 12, tile=21, blend=1))
    return c


CASES = _pitch_cases() + _ring_cases() + _flag_cases() + _geometry_cases() + _instance_cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ------------------------------------------------------------------------------------------------ data
def _seed(name):
    return zlib.crc32(name.encode())


def noise_volume(c):
    """(u8 VGH, f32 VGH, normals) of the case: [nz][ny][nx][3]"""
    nx, ny, nz = c["dims"]
    rng = np.random.default_rng(_seed(c["name"]))
    v8 = rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
    vf = rng.random((nz, ny, nx, 3), dtype=np.float32)
    if c["hole"]:   # a third of the slices stays inside the sparse table's clear band (values under 40 of 255)
        ax = {"z": 0, "y": 1, "x": 2}[c["pose"][0]]
        sl = [slice(None)] * 4
        sl[ax] = slice(c["ns"] // 3, 2 * c["ns"] // 3)
        sl[3] = 0
        v8[tuple(sl)] = v8[tuple(sl)] % 40
        vf[tuple(sl)] = vf[tuple(sl)] * np.float32(40.0 / 255.0)
    return v8, vf, O.normals_vgh(v8)


def dense_alpha(c):
    """the dense table's alpha bytes are drawn from [a, 2a]: about one optical depth over the case's planes"""
    return int(min(max(round(255.0 * 1.2 / c["steps"]), 2), 40))


def table2d(c, sparse):
    ts = c["tsize"]
    sv, sg = (ts, ts) if np.isscalar(ts) else ts
    rng = np.random.default_rng(_seed(c["name"]) ^ 0x7ab1e)
    a = dense_alpha(c)
    t = rng.integers(0, 256, (sg, sv, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(a, 2 * a + 1, (sg, sv), dtype=np.uint8)
    if sparse:
        t[..., 3] = np.minimum(t[..., 3].astype(np.int32) * 3, 255).astype(np.uint8)
        v = np.arange(sv) * 256 // sv
        t[:, (v < 44) | ((v >= 96) & (v < 128)) | ((v >= 200) & (v < 216)), 3] = 0     # bands of clear values
        g = np.arange(sg) * 256 // sg
        t[(g >= 64) & (g < 80), :, 3] = 0                                                # ... and of clear gradients
    return t


def table3d(c):
    rng = np.random.default_rng(_seed(c["name"]) ^ 0x3d)
    a = dense_alpha(c)
    t = rng.integers(0, 256, (16, 16, 16, 4), dtype=np.uint8)
    t[..., 3] = rng.integers(a, 2 * a + 1, (16, 16, 16), dtype=np.uint8)
    return t


def table_h(c):
    """the third axis's alpha texture (cfg 4): random, never clear"""
    rng = np.random.default_rng(_seed(c["name"]) ^ 0x4)
    t = np.zeros((256, 256, 4), np.uint8)
    t[..., 3] = rng.integers(128, 256, (1, 256), dtype=np.uint8)
    return t


def build_scene(c, volume=None):
    v8, vf, nrm = volume if volume is not None else noise_volume(c)
    ax = {"z": 2, "y": 1, "x": 0}[c["pose"][0]]
    fsize = [c["fill"]] * 3
    fsize[ax] = c["depth"]
    sc = O.Scene(vf if c["f32"] else v8, fsize=tuple(fsize), grad=nrm)
    kind = c["table"]
    if kind == "dense3d":
        sc.tf_mode = 2
        sc.tf3d = table3d(c)
    else:
        sc.tf_mode = 1
        sc.tf_vg = table2d(c, kind.startswith("sparse"))
        if kind.endswith("_h"):
            sc.tf_h = table_h(c)
            sc.third_axis = 1
    sc.width, sc.height = c["size"]
    sc.steps = c["steps"]
    sc.xform = O.rotation(*POSES[c["pose"]])
    sc.shade_mode = c["shade"]
    sc.frustum = tuple(f * c["frustum"] for f in sc.frustum)
    if c["feature"] == "shadows":
        sc.light_pos = (3, 4, -3)
        sc.shadow = (64, 0.7)
    return sc


def corner_drift(sc, perm):
    """|dU/dS| and |dV/dS| of the frame's corner rays, in voxels per slice (the planner's obliqueness measure)"""
    rc = sc.raycoef()
    au, av, as_ = {0: (0, 1, 2), 1: (0, 2, 1), 2: (1, 2, 0)}[perm]
    worst = 0.0
    for i in (0, sc.width - 1):
        for j in (0, sc.height - 1):
            px, py = (i + 0.5) * rc.pxs + rc.pxl, (j + 0.5) * rc.pys + rc.pyl
            B = [px * rc.Bx[a] + py * rc.By[a] + rc.Bc[a] for a in range(3)]
            worst = max(worst, abs(B[au] / B[as_]), abs(B[av] / B[as_]))
    return worst


# ------------------------------------------------------------------------------------------------ coverage
def stored_extents(c, perm):
    """(Du, Dv) of the stored box along the plan's U and V, in voxels (u8 rows are padded to an even length)"""
    nx, ny, nz = c["dims"]
    du, dv = {0: (nx, ny), 1: (nx, nz), 2: (ny, nz)}[perm]
    return du, dv


def tally(records):
    """records: [(case, plan dict)].  Returns (rows, missing): the reached classes as printable rows, and what the issue
    asks for that no record reaches."""
    rows, missing = [], []

    def need(what, ok, detail=""):
        rows.append("%-46s %s%s" % (what, "ok" if ok else "MISSING", (" " + detail) if detail else ""))
        if not ok:
            missing.append(what)

    recs = [dict(p, case=c, f32=c["f32"], big=p["nw"] + p["nl"] > 12, sparse=c["table"].startswith("sparse"),
                 Dv=stored_extents(c, p["perm"])[1], Du=stored_extents(c, p["perm"])[0],
                 ntx=-(-c["size"][0] // p["tw"]), nty=-(-c["size"][1] // p["th"])) for c, p in records]
    some = lambda f: [r for r in recs if f(r)]                                                              # noqa: E731
    # -- pitch
    classes = [4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64]
    for wp in classes:
        for f32 in (True, False):
            if not f32 and wp > 32:
                continue
            mine = some(lambda r: r["wp"] == wp and r["f32"] == f32)
            tag = "pitch %2d %s" % (wp, "f32" if f32 else "u8 ")
            if wp != 64:   # (64: one row to the group and at least two rows to a window -- test_gpu_slab_plans.py's docstring)
                need(tag + " groups == 1", any(r["groups"] == 1 for r in mine))
            need(tag + " groups >= 3", any(r["groups"] >= 3 for r in mine))
            need(tag + " wu == wp", any(r["wu"] == wp for r in mine))
            need(tag + " wu < wp", any(r["wu"] < wp for r in mine))
    need("ragged last group, big workgroup", bool(some(lambda r: r["big"] and r["wv"] % r["rpg"])))
    need("ragged last group, small workgroup", bool(some(lambda r: not r["big"] and r["wv"] % r["rpg"] and r["groups"] * r["rpg"] > r["Dv"])))
    # -- axes, directions, shapes
    for perm in (0, 1, 2):
        need("perm %d at per > 1" % perm, bool(some(lambda r: r["perm"] == perm and r["per"] > 1)))
    for d in (1, -1):
        need("dir %+d at per > 1" % d, bool(some(lambda r: r["dir"] == d and r["per"] > 1)))
    for tile in sorted(TILES):
        need("tile %2d at per > 1" % tile, bool(some(lambda r: r["case"]["tile"] == tile and r["per"] > 1)))
    need("tile 0 (the planner's choice)", bool(some(lambda r: r["case"]["tile"] == 0)))
    for big in (False, True):
        for sparse in (False, True):
            need("%s workgroup, %s table" % ("big" if big else "small", "sparse" if sparse else "dense"),
                 bool(some(lambda r: r["big"] == big and r["sparse"] == sparse)))
    # -- ring
    need("nslots == 3 forced (slab_ns)", bool(some(lambda r: r["nslots"] == 3 and r["case"]["opts"].get("slab_ns") == 3)))
    need("nslots == 3 natural", bool(some(lambda r: r["nslots"] == 3 and "slab_ns" not in r["case"]["opts"])))
    need("nslots == 24", bool(some(lambda r: r["nslots"] == 24)))
    need("3 < nslots < 24", bool(some(lambda r: 3 < r["nslots"] < 24)))
    need("slices < nslots", bool(some(lambda r: r["slices_max"] < r["nslots"])))
    need("slices == nslots", bool(some(lambda r: r["slices_max"] == r["nslots"])))
    need("slices > nslots", bool(some(lambda r: r["slices_max"] > r["nslots"])))
    need("slices > 64 at per > 1", bool(some(lambda r: 64 < r["slices_max"] <= 128 and r["per"] > 1)))
    need("slices > 128 at per > 1", bool(some(lambda r: r["slices_max"] > 128 and r["per"] > 1)))
    need("maxfly == 1", bool(some(lambda r: r["maxfly"] == 1)))
    need("maxfly == 2", bool(some(lambda r: r["maxfly"] == 2)))
    need("maxfly >= 3 (slab_fly)", bool(some(lambda r: r["maxfly"] >= 3 and r["case"]["opts"].get("slab_fly", 0) >= 3)))
    need("maxfly bound by 63 // mych + 1, mych >= 32",
         bool(some(lambda r: r["mych"] >= 32 and r["maxfly"] == 63 // r["mych"] + 1 < min(r["nslots"], r["case"]["opts"].get("slab_fly", 0)))))
    small_max = max([r["mych"] for r in recs if not r["big"]] or [0])
    big_max = max([r["mych"] for r in recs if r["big"]] or [0])
    need("largest mych, small workgroup (52)", small_max == 52, "found %d" % small_max)
    need("largest mych, big workgroup (28)", big_max == 28, "found %d" % big_max)
    need("wstep == 0", bool(some(lambda r: r["wstep"] == 0)))
    need("wstep == 0 by slab_T 1", bool(some(lambda r: r["wstep"] == 0 and r["case"]["opts"].get("slab_T") == 1)))
    need("wstep == 1", bool(some(lambda r: r["wstep"] == 1)))
    need("wstep >= 2", bool(some(lambda r: r["wstep"] >= 2)))
    need("wstep >= 2 by slab_T", bool(some(lambda r: r["wstep"] >= 2 and r["case"]["opts"].get("slab_T", 0) >= 3)))
    for v in (0, 1):
        need("pmask == %d" % v, bool(some(lambda r: r["pmask"] == v)))
        need("mask_need == %d" % v, bool(some(lambda r: r["mask_need"] == v)))
        need("use_occ == %d" % v, bool(some(lambda r: r["use_occ"] == v)))
        need("use_ah == %d" % v, bool(some(lambda r: r["use_ah"] == v)))
        need("bricks == %d on the sparse table (option bricks %d)" % (v, v),
             bool(some(lambda r: r["sparse"] and r["bricks"] == v and r["case"]["opts"].get("bricks", 1) == v)))
        need("3-D table, use_occ == %d" % v, bool(some(lambda r: r["case"]["table"] == "dense3d" and r["use_occ"] == v)))
    # -- geometry
    need("two slices along the marching axis", bool(some(lambda r: r["case"]["ns"] == 2)))
    need("three slices along the marching axis", bool(some(lambda r: r["case"]["ns"] == 3)))
    need("wv == the stored extent", bool(some(lambda r: r["wv"] == r["Dv"])))
    need("several tiles, windows clamped at both faces",
         bool(some(lambda r: r["ntx"] >= 2 and r["nty"] >= 2 and r["wu"] * (1 if r["f32"] else 2) < r["Du"] and r["wv"] < r["Dv"]
                   and r["case"]["fill"] < 1.0)))
    need("close-up, drift over 2 voxels per slice", bool(some(lambda r: r.get("drift", 0) > 2.0)))
    need("odd window size", bool(some(lambda r: r["case"]["size"][0] % 2 and r["case"]["size"][1] % 2 and r["ntx"] * r["nty"] > 1)))
    for f in ("shadows", "occluded", "depth"):
        need("%s at per > 1" % f, bool(some(lambda r: r["case"]["feature"] == f and r["per"] > 1)))
    need("forced depth segments at per > 1", bool(some(lambda r: r["case"]["opts"].get("slab_split") == 3 and r["per"] > 1)))
    need("x-major copy (perm 2)", bool(some(lambda r: r["perm"] == 2)))
    return rows, missing


# ---- the plans the cases were dialled to (the read-back of every case; lds_bytes left out: it follows from the rest)
_PLAN_KEYS = [f for f in PLAN_FIELDS if f != "lds_bytes"]
_PLAN_ROWS = {
    # tw th nw nl wu wv wp per rpg groups chunks mych nslots maxfly wstep pmask mask_need use_occ use_ah fast_tf bricks perm dir slices_max
    "p4-f32-g1":             (32, 16, 8, 2, 4, 16, 4, 1, 16, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 2, -1, 6),
    "p4-f32-g3":             (24, 32, 12, 4, 3, 40, 4, 1, 16, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 2, 1, 11),
    "p4-u8-g1":              (40, 16, 10, 2, 4, 16, 4, 1, 16, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 16),
    "p4-u8-g3":              (32, 24, 12, 4, 3, 40, 4, 1, 16, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 1, -1, 21),
    "p8-f32-g1":             (16, 32, 8, 2, 8, 8, 8, 1, 8, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 26),
    "p8-f32-g3":             (48, 16, 12, 4, 7, 20, 8, 1, 8, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 0, -1, 31),
    "p8-u8-g1":              (16, 40, 10, 2, 8, 8, 8, 1, 8, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 2, -1, 36),
    "p8-u8-g3":              (16, 48, 12, 4, 7, 20, 8, 1, 8, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 2, 1, 6),
    "p12-f32-g1":            (40, 16, 10, 2, 12, 16, 12, 3, 16, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 11),
    "p12-f32-g3":            (48, 16, 12, 4, 11, 40, 12, 3, 16, 3, 9, 6, 16, 2, 1, 1, 1, 1, 0, 1, 0, 1, -1, 16),
    "p12-u8-g1":             (32, 16, 8, 2, 12, 16, 12, 3, 16, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 21),
    "p12-u8-g3":             (24, 32, 12, 4, 11, 40, 12, 3, 16, 3, 9, 6, 16, 2, 1, 1, 1, 1, 0, 1, 0, 0, -1, 26),
    "p16-f32-g1":            (40, 16, 10, 2, 16, 4, 16, 1, 4, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 2, -1, 31),
    "p16-f32-g3":            (32, 24, 12, 4, 15, 11, 16, 1, 4, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 2, 1, 36),
    "p16-u8-g1":             (16, 32, 8, 2, 16, 4, 16, 1, 4, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 6),
    "p16-u8-g3":             (48, 16, 12, 4, 15, 11, 16, 1, 4, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 1, -1, 11),
    "p20-f32-g1":            (16, 40, 10, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 16),
    "p20-f32-g3":            (16, 48, 12, 4, 19, 44, 20, 5, 16, 3, 15, 10, 9, 2, 1, 1, 1, 1, 0, 1, 0, 0, -1, 21),
    "p20-u8-g1":             (40, 16, 10, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 1, 1, 1, 1, 0, 1, 0, 2, -1, 26),
    "p20-u8-g3":             (48, 16, 12, 4, 19, 44, 20, 5, 16, 3, 15, 10, 9, 2, 1, 1, 1, 1, 0, 1, 0, 2, 1, 31),
    "p24-f32-g1":            (32, 16, 8, 2, 24, 8, 24, 3, 8, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 36),
    "p24-f32-g3":            (24, 32, 12, 4, 23, 20, 24, 3, 8, 3, 9, 6, 16, 2, 1, 1, 1, 1, 0, 1, 0, 1, -1, 6),
    "p24-u8-g1":             (40, 16, 10, 2, 24, 8, 24, 3, 8, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 11),
    "p24-u8-g3":             (32, 24, 12, 4, 23, 20, 24, 3, 8, 3, 9, 6, 16, 2, 1, 1, 1, 1, 0, 1, 0, 0, -1, 16),
    "p28-f32-g1":            (16, 32, 8, 2, 28, 16, 28, 7, 16, 1, 7, 7, 9, 1, 1, 1, 1, 1, 0, 1, 0, 2, -1, 21),
    "p28-f32-g3":            (48, 16, 12, 4, 27, 44, 28, 7, 16, 3, 21, 14, 7, 2, 1, 1, 1, 1, 0, 1, 0, 2, 1, 26),
    "p28-u8-g1":             (16, 40, 10, 2, 28, 16, 28, 7, 16, 1, 7, 7, 9, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 31),
    "p28-u8-g3":             (16, 48, 12, 4, 27, 44, 28, 7, 16, 3, 21, 14, 7, 2, 1, 1, 1, 1, 0, 1, 0, 1, -1, 36),
    "p32-f32-g1":            (40, 16, 10, 2, 32, 2, 32, 1, 2, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 6),
    "p32-f32-g3":            (48, 16, 12, 4, 31, 5, 32, 1, 2, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 0, -1, 11),
    "p32-u8-g1":             (32, 16, 8, 2, 32, 2, 32, 1, 2, 1, 1, 1, 24, 1, 1, 1, 0, 0, 0, 1, 0, 2, -1, 16),
    "p32-u8-g3":             (24, 32, 12, 4, 31, 5, 32, 1, 2, 3, 3, 2, 24, 2, 1, 1, 0, 0, 0, 1, 0, 2, 1, 21),
    "p40-f32-g1":            (40, 16, 10, 2, 40, 8, 40, 5, 8, 1, 5, 5, 13, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 26),
    "p40-f32-g3":            (32, 24, 12, 4, 39, 20, 40, 5, 8, 3, 15, 10, 9, 2, 1, 1, 1, 1, 0, 1, 0, 1, -1, 31),
    "p48-f32-g1":            (16, 32, 8, 2, 48, 4, 48, 3, 4, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 36),
    "p48-f32-g3":            (48, 16, 12, 4, 47, 11, 48, 3, 4, 3, 9, 6, 16, 2, 1, 1, 1, 1, 0, 1, 0, 0, -1, 6),
    "p56-f32-g1":            (16, 40, 10, 2, 56, 8, 56, 7, 8, 1, 7, 7, 9, 1, 1, 1, 1, 1, 0, 1, 0, 2, -1, 11),
    "p56-f32-g3":            (16, 48, 12, 4, 55, 20, 56, 7, 8, 3, 21, 14, 7, 2, 1, 1, 1, 1, 0, 1, 0, 2, 1, 16),
    "p64-f32-g1":            (40, 16, 10, 2, 64, 3, 64, 1, 1, 3, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 1, 1, 21),
    "p64-f32-g3":            (48, 16, 12, 4, 63, 5, 64, 1, 1, 5, 5, 3, 24, 2, 1, 1, 1, 1, 0, 1, 0, 1, -1, 26),
    "ring24-eq":             (32, 16, 8, 2, 12, 16, 12, 3, 16, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 24),
    "ring3-forced":          (16, 32, 8, 2, 12, 16, 12, 3, 16, 1, 3, 3, 3, 1, 0, 0, 0, 0, 0, 1, 0, 1, -1, 40),
    "ring3-natural-small":   (40, 16, 10, 2, 56, 56, 56, 7, 8, 7, 49, 49, 3, 2, 0, 0, 1, 1, 0, 1, 0, 0, -1, 9),
    "mych-max-big":          (32, 24, 12, 4, 56, 56, 56, 7, 8, 7, 49, 28, 3, 2, 0, 0, 1, 1, 0, 1, 0, 0, 1, 9),
    "mych-max-small":        (40, 16, 10, 2, 64, 52, 64, 1, 1, 52, 52, 52, 3, 1, 0, 0, 1, 1, 0, 1, 0, 1, 1, 7),
    "stick-100":             (16, 32, 8, 2, 24, 8, 24, 3, 8, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 1, 2, -1, 100),
    "stick-200":             (32, 16, 8, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 5, 0, 1, 1, 0, 1, 0, 0, -1, 200),
    "stick-200-u8":          (32, 24, 12, 4, 20, 16, 20, 5, 16, 1, 5, 5, 24, 2, 2, 1, 1, 1, 0, 1, 1, 1, 1, 150),
    "stick-fly3":            (16, 40, 10, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 3, 1, 1, 1, 1, 0, 1, 0, 2, 1, 70),
    "stick-T1":              (24, 32, 12, 4, 24, 8, 24, 3, 8, 1, 3, 3, 24, 2, 0, 1, 0, 0, 0, 1, 0, 0, 1, 70),
    "stick-T2":              (48, 16, 12, 4, 24, 8, 24, 3, 8, 1, 3, 3, 24, 2, 1, 1, 0, 0, 0, 1, 0, 1, -1, 70),
    "stick-T3":              (40, 16, 10, 2, 24, 8, 24, 3, 8, 1, 3, 3, 24, 1, 2, 1, 0, 0, 0, 1, 0, 0, -1, 70),
    "third-axis":            (32, 16, 8, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 12),
    "third-axis-u8":         (32, 24, 12, 4, 20, 44, 20, 5, 16, 3, 15, 10, 9, 2, 1, 1, 1, 1, 1, 1, 0, 2, -1, 12),
    "bricks-off":            (40, 16, 10, 2, 24, 20, 24, 3, 8, 3, 9, 9, 7, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 30),
    "bricks-on":             (40, 16, 10, 2, 24, 20, 24, 3, 8, 3, 9, 9, 7, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 30),
    "big-table":             (32, 16, 8, 2, 24, 20, 24, 3, 8, 3, 9, 9, 8, 1, 1, 1, 1, 0, 0, 1, 0, 0, -1, 10),
    "tf3d-occ":              (16, 32, 8, 2, 24, 20, 24, 3, 8, 3, 9, 9, 8, 1, 1, 1, 1, 1, 0, 0, 0, 2, 1, 10),
    "tf3d-noocc":            (32, 16, 8, 2, 12, 16, 12, 3, 16, 1, 3, 3, 24, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 10),
    "tf3d-u8":               (16, 48, 12, 4, 20, 16, 20, 5, 16, 1, 5, 5, 24, 2, 1, 1, 1, 1, 0, 0, 0, 1, -1, 10),
    "two-slices":            (32, 16, 8, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 2),
    "three-slices":          (16, 32, 8, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 1, 1, 1, 1, 0, 1, 0, 1, -1, 3),
    "three-slices-u8":       (40, 16, 10, 2, 12, 12, 16, 1, 4, 3, 3, 3, 24, 1, 1, 1, 0, 0, 0, 1, 0, 2, -1, 3),
    "tiles-2x3":             (32, 16, 8, 2, 40, 32, 40, 5, 8, 4, 20, 20, 7, 1, 1, 1, 1, 1, 0, 1, 0, 0, 1, 20),
    "tiles-auto-odd":        (32, 24, 12, 4, 35, 37, 40, 5, 8, 5, 25, 15, 5, 2, 1, 0, 1, 1, 0, 1, 0, 1, 1, 24),
    "tiles-big-u8":          (24, 32, 12, 4, 21, 39, 24, 3, 8, 5, 15, 9, 9, 2, 1, 1, 1, 1, 0, 1, 0, 2, 1, 16),
    "tiles-big-f32":         (32, 24, 12, 4, 44, 45, 48, 3, 4, 12, 36, 18, 4, 2, 0, 0, 1, 1, 0, 1, 0, 0, -1, 16),
    "closeup":               (32, 16, 8, 2, 40, 40, 40, 5, 8, 5, 25, 25, 5, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 4),
    "shadows":               (32, 16, 8, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 2, 1, 1, 1, 0, 1, 0, 0, 1, 12),
    "occluded":              (16, 32, 8, 2, 24, 20, 24, 3, 8, 3, 9, 9, 7, 1, 1, 1, 1, 1, 0, 1, 0, 1, 1, 12),
    "split3":                (40, 16, 10, 2, 28, 16, 28, 7, 16, 1, 7, 7, 9, 1, 1, 1, 1, 1, 0, 1, 0, 2, -1, 40),
    "first-hit-depth":       (32, 24, 12, 4, 40, 20, 40, 5, 8, 3, 15, 10, 9, 2, 1, 1, 1, 1, 0, 1, 0, 0, -1, 12),
    "back-to-front":         (16, 40, 10, 2, 20, 16, 20, 5, 16, 1, 5, 5, 13, 1, 1, 1, 1, 1, 0, 1, 0, 1, -1, 12),
}
PLANS = {k: dict(zip(_PLAN_KEYS, v)) for k, v in _PLAN_ROWS.items()}
