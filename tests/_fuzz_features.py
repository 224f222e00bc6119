"""The feature fuzz's generator: seeded random frames over every frame feature the three ray-marchers take -- the six
classifications, both voxel types, shading, the three blend modes, first-hit depth, the four ways of cutting the box
(orthogonal clip, free clip plane, sub-box, shard) and perturbation -- on the small ragged volumes, odd windows and
close-up / panned / asymmetric views that have broken kernels here.

    feat = draw(seed, case)          the feature record: plain numbers, no arrays, cheap
    sc = build(feat)                 the oracle.Scene of that record
    sc, feat = feature_scene(seed, case)

A case draws from np.random.default_rng([seed, case]) alone, so it is reproducible without the cases before it
(tools/fuzz_one.py --features SEED CASE).  tests/test_fuzz_features_cpu.py holds the generator, at the default seed
and NCASES, to its coverage, to frames that show something and to the share of cases the column-stream kernel takes by
mode; tests/test_gpu_fuzz_features.py renders the cases.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

import _scenes as S
from _scenes import O

NCASES = int(os.environ.get("SMK_FUZZ_CASES", "48"))
DEFAULT_SEED, DEFAULT_NCASES = 18, 48
SEED = int(os.environ.get("SMK_FUZZ_SEED", str(DEFAULT_SEED)))

KINDS = ("cfg1", "cfg2", "cfg3", "cfg4", "tf3d", "tf3d_panes")
CUTS = ("none", "clip", "plane", "region", "shard")
VIEWS = ("default", "closeup", "pan", "asym")
# shares: the column-stream kernel takes by mode what has no perturbation, no back-to-front blend and no free plane --
# .85 x .80 x .86 = 58 % expected, 40 % asserted (test_fuzz_features_cpu.py)
P_PERT, P_BLEND, P_CUT, P_DEPTH = 0.15, (0.5, 0.2, 0.3), (0.38, 0.16, 0.14, 0.16, 0.16), 0.4
P_VIEW = (0.5, 0.2, 0.2, 0.1)


def _f(x):
    return float(x)


def draw(seed, case):
    rng = np.random.default_rng([int(seed), int(case)])
    ft = dict(seed=int(seed), case=int(case))
    hi = 72 if rng.random() < 0.25 else 40
    dims = [int(rng.integers(2, hi + 1)) for _ in range(3)]
    if rng.random() < 0.2:                      # a slab-shaped volume: one axis very thin
        dims[int(rng.integers(0, 3))] = int(rng.integers(2, 5))
    ft["vol_seed"] = int(rng.integers(1, 1000))
    ft["kind"] = KINDS[int(rng.integers(0, len(KINDS)))]
    ft["f32"] = bool(rng.integers(0, 2)) and ft["kind"] != "cfg1"     # (cfg1 is the u8 scalar volume)
    ft["h_slider"] = _f(rng.uniform(0.2, 0.8))
    ft["shade"] = 0 if ft["kind"] == "cfg1" else int(rng.integers(0, 3))
    ft["use_spec"] = int(rng.integers(0, 2))
    ft["blend"] = int(rng.choice(3, p=P_BLEND))
    ft["depth"] = bool(rng.random() < P_DEPTH)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis) + 1e-9
    ft["rot"] = (tuple(_f(a) for a in axis), _f(rng.uniform(-180, 180)))
    ft["width"], ft["height"] = int(rng.integers(9, 150)), int(rng.integers(9, 150))
    if ft["width"] == ft["height"]:
        ft["height"] += 1
    ft["steps"], ft["rate"] = int(rng.integers(6, 161)), 0.0
    if rng.random() < 0.15:
        ft["steps"], ft["rate"] = 0, _f(rng.uniform(0.3, 2.5))
    ft["view"] = VIEWS[int(rng.choice(4, p=P_VIEW))]
    ft["eye"], ft["trans"], ft["frustum"] = None, None, None
    if ft["view"] == "closeup":                 # strong perspective, part of the volume off screen
        ft["eye"] = (_f(rng.uniform(-.3, .3)), _f(rng.uniform(-.3, .3)), -_f(rng.uniform(1.6, 2.5)))
        w = _f(rng.uniform(0.15, 0.45))
        ft["frustum"] = (-w, w, -w, w)
    elif ft["view"] == "pan":
        ft["trans"] = (_f(rng.uniform(-.6, .6)), _f(rng.uniform(-.6, .6)), _f(rng.uniform(-1, 1)))
    elif ft["view"] == "asym":
        ft["frustum"] = (-0.03, 0.11, -0.09, 0.05)
    # ---- the cut: at most one
    ft["cut"] = CUTS[int(rng.choice(len(CUTS), p=P_CUT))]
    ft["clip"] = ft["plane"] = ft["region"] = ft["shard"] = None
    u = rng.random(8)
    if ft["cut"] == "clip":                     # the clip-plane widget in its orthogonal mode: (axis 1..6, position / fsize)
        ft["clip"] = (1 + int(u[0] * 6), tuple(0.1 + 0.8 * _f(v) for v in u[1:4]))
    elif ft["cut"] == "plane":                  # eye-space normal, a point of the box's middle 60 % (as fractions), the side
        n = rng.normal(size=3)
        n /= np.linalg.norm(n) + 1e-9
        ft["plane"] = (tuple(_f(v) for v in n), tuple(0.2 + 0.6 * _f(v) for v in u[1:4]), 1 if u[4] < 0.5 else -1)
    elif ft["cut"] == "shard":                  # one rank's brick region of a sort-last job: every split axis >= 4 voxels
        world = int(rng.choice([2, 4, 8]))
        for bit in range(world.bit_length() - 1):
            dims[bit] = max(dims[bit], 4)
        ft["shard"] = (int(rng.integers(0, world)), world)
    elif ft["cut"] == "region":                 # a sub-box that is no shard: >= 2 voxels and at least a third of each axis
        g0, g1 = [], []
        for a in range(3):
            n = int(rng.integers(max(2, dims[a] // 3), dims[a] + 1))
            lo = int(rng.integers(0, dims[a] - n + 1))
            g0.append(lo)
            g1.append(lo + n)
        if g0 == [0, 0, 0] and g1 == dims:      # (drew the whole box: halve the longest axis)
            a = int(np.argmax(dims))
            if dims[a] >= 4:
                g1[a] = max(2, dims[a] // 2)
            else:
                ft["cut"] = "none"
        if ft["cut"] == "region":
            ft["region"] = (tuple(g0), tuple(g1))
    ft["dims"] = tuple(dims)
    ft["thin"] = min(dims) <= 4
    ft["pert"] = bool(rng.random() < P_PERT)
    ft["pert_w"] = (_f(rng.uniform(0, .3)), _f(rng.uniform(0, .2)), 0.0, 0.0)
    return ft


def cols_by_mode(ft):
    """what the column-stream kernel takes as far as modes go (cols_refusal, smk_cols_plan.hip; depth is not requested there)"""
    return not ft["pert"] and ft["blend"] != 1 and ft["cut"] != "plane"


def volume(dims, seed):
    """S.ragged_vgh's field, cut out of one a voxel larger on every side: make_vgh zeroes a volume's outermost voxels (a 2-voxel
    axis would be empty, a 3-voxel one a single sheet), here the data reach the faces of the box"""
    big = S.ragged_vgh(tuple(d + 2 for d in dims), seed=seed)
    return tuple(np.ascontiguousarray(a[1:-1, 1:-1, 1:-1]) for a in big)


def build(ft, cut=True):
    """the oracle.Scene of a feature record; cut=False: the same frame without its cut"""
    dims = ft["dims"]
    vgh8, vghf, nrm = volume(dims, ft["vol_seed"])
    kind = ft["kind"]
    if kind == "cfg1":
        sc = O.Scene(np.ascontiguousarray(vgh8[..., :1]))
        sc.tf_mode, sc.tlut = 0, O.tlut_volumerenderable()
    else:
        sc = O.Scene(vghf if ft["f32"] else vgh8, grad=nrm)
        sc.tf_mode = 1
        if kind == "cfg2":
            sc.tf_vg, sc.tf_h = S.tf_cfg2()
        elif kind in ("cfg3", "cfg4"):
            sc.tf_vg = S.tf_cfg3()
            if kind == "cfg4":
                sc.tf_h, sc.third_axis = S.tf_h(ft["h_slider"]), 1
        else:
            sc.tf_mode, sc.tf3d = 2, (S.tf3d_dense() if kind == "tf3d" else S.tf3d_panes())
    sc.xform = O.rotation(*ft["rot"])
    sc.width, sc.height = ft["width"], ft["height"]
    sc.steps, sc.sample_rate = ft["steps"], ft["rate"]
    sc.shade_mode, sc.use_spec = ft["shade"], ft["use_spec"]
    if ft["eye"]:
        sc.eye = ft["eye"]
    if ft["trans"]:
        sc.trans = ft["trans"]
    if ft["frustum"]:
        sc.frustum = ft["frustum"]
    sc.blend = ft["blend"]
    sc.shard = None
    sc.subbox = False
    if cut and ft["clip"]:
        sc.clip = (ft["clip"][0], tuple(f * _f(s) for f, s in zip(ft["clip"][1], sc.fsize)))
    if cut and ft["plane"]:
        n, frac, side = ft["plane"]
        mv = np.array(sc.mv(), np.float64).reshape(4, 4).T
        pe = mv @ np.array([frac[0] * _f(sc.fsize[0]), frac[1] * _f(sc.fsize[1]), frac[2] * _f(sc.fsize[2]), 1.0])
        n = side * np.array(n)
        sc.clip_plane = (_f(n[0]), _f(n[1]), _f(n[2]), -_f(n @ pe[:3]))
    if cut and ft["region"]:
        sc.region, sc.subbox = ft["region"], True
    if cut and ft["shard"]:
        from conftest import load_package
        load_package()
        from simian_spacemonkey_amd import sortlast
        sc.shard = ft["shard"]
        sc.region = sortlast.shard_region(sc.dims, *sc.shard)
    if ft["pert"]:
        sc.noise = O.noise_tex(32)
        sc.pert_w = ft["pert_w"]
        sc.pert_s = (.2, 2.1, 4.5, 8.7)
    return sc


def feature_scene(seed, case):
    ft = draw(seed, case)
    return build(ft), ft


def halo_for(ft):
    """the halo a sharded context needs for this case's displaced fetches (smk_build_params states the rule), else None"""
    if not (ft["pert"] and ft["shard"]):
        return None
    return max(2 + int(np.ceil(0.5 * (abs(ft["pert_w"][0]) + abs(ft["pert_w"][1])) * n)) for n in ft["dims"])


def describe(ft):
    cut = {"none": "", "clip": " clip %s" % (ft["clip"],), "plane": " plane %s" % (ft["plane"],), "region": " region %s" % (ft["region"],),
           "shard": " shard %s" % (ft["shard"],)}[ft["cut"]]
    return "case %d (seed %d): %s %s dims %s %dx%d x%d rate %.2f shade %d spec %d blend %d depth %d view %s pert %d%s" % (
        ft["case"], ft["seed"], ft["kind"], "f32" if ft["f32"] else "u8", ft["dims"], ft["width"], ft["height"], ft["steps"], ft["rate"],
        ft["shade"], ft["use_spec"], ft["blend"], ft["depth"], ft["view"], ft["pert"], cut)
