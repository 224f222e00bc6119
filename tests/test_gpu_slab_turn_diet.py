"""A consumer's turn of the slice-ring kernel after the compiler's bookkeeping was taken out of it (DESIGN.md section 4,
*Instruction stream of a turn*): the wave minimum with the DPP modifier on the v_min itself and a row_bcast finish, `work`
as a lane mask, and fetch, normal, alpha, colour, shading, first-hit depth and blend as ONE block behind the occupancy bit.
None of it touches an operation on data, so none of it may change a bit of a frame.

What could go wrong, and the smallest frames that show it:
  * a wave minimum that is too high recycles a ring slot that a slower lane still reads.  The ring forced to its shortest
    (slab_ns 3: a progress word every turn, slab_plan_pmask 0) has no slack to hide that; the deep ring publishes every other
    turn (pmask 1); the 12 + 4-wave workgroups take the minimum of the NEXT positions every turn.  The view is turned 0, 90,
    180 and 270 degrees about its own axis under each of the six marching directions, so that the wave's slowest lane falls
    into every DPP row and bank of the reduction;
  * a wrong `work` mask samples a layer whose slices were never streamed, or skips one that shows: a table with clear
    bands over a volume whose middle third lies inside them, brick flags on -- the planner keeps them, asserted -- against
    the same frame with option bricks 0;
  * a variant of the nested block that lost a step: the separable 2-D table without and with the third-axis alpha, the
    dense 3-D table with its bitmap, first-hit depth, the GL_MAX blend.

The condition is the suite's: every slice-ring frame (option kernel 2: a declined frame raises, nothing falls back) equals
the gather kernel's bit for bit -- it shares none of the edited code -- and so does the same frame with option bricks 0;
last_frame_info()[0] == 2 and slab_failures == 0 in every case.

Data: per-voxel noise seeded by the case's name under tables in which every texel counts (tests/_slab_plan_cases.py), so a
voxel, texel or table entry fetched from a wrong place holds other numbers than the right one.  24^3 voxels for the
wave-minimum sweep, 40^3 where whole layers of bricks must come out empty; 64 x 48 pixels, 48 planes: several tiles of every
shape, several waves a tile, more slices than the short ring holds."""
import functools

import numpy as np
import pytest

import oracle as O
import _u16_ref as U
from _scenes import push_scene
from _slab_plan_cases import POSES as POSE_AXES
from _slab_plan_cases import build_scene, case, noise_volume

pytestmark = pytest.mark.gpu
VOXELS = ("f32", "u8", "u16")
POSES = ("z+", "z-", "y+", "y-", "x+", "x-")
ROLLS = (0, 90, 180, 270)
RINGS = (3, 0)                        # option slab_ns: the shortest ring, and the planner's own (deep at these sizes)
SHAPES = ((5, (8, 2)), (20, (10, 2)), (4, (12, 4)))   # option tile -> consumer + loader waves
UPRIGHT = {5: 7, 20: 21, 4: 2}        # the same shapes with the tile's sides swapped (32 x 16 -> 16 x 32, ...)
KNOBS = (("kernel", 0), ("bricks", 1), ("tile", 0), ("slab_ns", 0))


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _restore(R):
    yield
    for k, v in KNOBS:
        R.set_option(k, v)
    R.set_blend(0)


def _case(n, pose, table):
    return case("turn-%d-%s" % (n, pose), pose, n, n, n, table=table, hole=table.startswith("sparse"), size=(64, 48), steps=48,
                fill=0.9, depth=0.9, shade=1)


@functools.lru_cache(maxsize=None)
def _volume(n, pose, hole):
    """(u8 VGH, f32 VGH, normals); hole: the middle third of the slices along the marching axis lies in the clear band"""
    v8, vf, nrm = noise_volume(_case(n, pose, "sparse" if hole else "dense"))
    for a in (v8, vf, nrm):
        a.setflags(write=False)
    return v8, vf, nrm


def _matrix(xform):
    return np.asarray(xform, np.float64).reshape(4, 4).T   # (column-major list -> matrix)


@functools.lru_cache(maxsize=None)
def _scene(voxels, n, pose, table, roll=0):
    """what a push needs of the case: the checker's scene object carries the frame state, nothing is rendered on the CPU"""
    c = _case(n, pose, table)
    v8, vf, nrm = _volume(n, pose, c["hole"])
    vol16 = None
    if voxels == "u16":   # the same noise as 16-bit integers; the scene holds their decoded values
        vol16 = np.ascontiguousarray((vf.astype(np.float64) * 65535.0).astype(np.uint16))
        vf = U.decode_u16(vol16)
    sc = build_scene(dict(c, f32=voxels != "u8"), volume=(v8, vf, nrm))
    if roll:              # the eye looks down the world's z axis: a turn about it, applied after the pose, rolls the image
        m = _matrix(O.rotation((0, 0, 1), roll)) @ _matrix(O.rotation(*POSE_AXES[pose]))
        sc.xform = [float(v) for v in m.T.reshape(-1)]
    if vol16 is not None:
        sc.dmode = "VGH"
        return U.Case(vol16, sc)
    return sc


def _push(R, s):
    if isinstance(s, U.Case):
        U.push(R, s)
    else:
        push_scene(R, s)


def _frames(R, tile, ring, blend=0, **kw):
    """the frame on the gather kernel, on the forced slice-ring kernel with brick flags, and on it without; the plan of
    the frame with flags"""
    assert R.stat("slab_failures") == 0
    R.set_blend(blend)
    R.set_option("bricks", 1)
    R.set_option("kernel", 1)
    g = R.render(**kw)
    assert R.last_frame_info()[0] == 1
    R.set_option("kernel", 2)          # raises where the slice-ring kernel declines the frame
    R.set_option("tile", tile)
    R.set_option("slab_ns", ring)
    out = []
    for bricks in (0, 1):
        R.set_option("bricks", bricks)
        out.append(R.render(**kw))
        assert R.last_frame_info()[0] == 2, "the frame was declined"
        assert R.stat("slab_status") == 0
        assert R.stat("slab_failures") == 0 and R.stat("slab_retries") == 0
    plan = {f: int(R.stat("slab_plan_" + f)) for f in ("nw", "nl", "nslots", "pmask", "bricks", "use_occ", "use_ah", "fast_tf")}
    return g, out[1], out[0], plan


def _same(a, b, what):
    assert np.array_equal(a, b), "%s: differs by %g in %d pixels" % (what, np.abs(a - b).max(), (a != b).any(-1).sum())


def _check_ring(plan, ring, shape):
    assert (plan["nw"], plan["nl"]) == shape, plan
    if ring == 3:
        assert plan["nslots"] == 3 and plan["pmask"] == 0, plan
    else:
        assert plan["nslots"] > 3 and plan["pmask"] == 1, plan


# ---- the wave minimum: marching direction x roll x ring x workgroup shape, the voxel type taking turns; the quarter turns
# of the view run on the tiles with their sides swapped, so both orientations of every shape are marched
_MIN = [(VOXELS[(ip + ir + it) % 3], pose, roll, ring, UPRIGHT[tile] if roll % 180 else tile, shape)
        for ip, pose in enumerate(POSES) for ir, roll in enumerate(ROLLS) for ring in RINGS for it, (tile, shape) in enumerate(SHAPES)]


@pytest.mark.parametrize("voxels,pose,roll,ring,tile,shape", _MIN,
                         ids=["%s-%s-r%d-ns%d-t%d-%d+%d" % (v, p, ro, ri, t, s[0], s[1]) for v, p, ro, ri, t, s in _MIN])
def test_wave_minimum(R, voxels, pose, roll, ring, tile, shape):
    _push(R, _scene(voxels, 24, pose, "dense", roll))
    g, s, s0, plan = _frames(R, tile, ring)
    _check_ring(plan, ring, shape)
    assert s[..., 3].max() > 0.05, "the frame shows nothing"
    _same(g, s, "against the gather kernel")
    _same(s, s0, "against the frame with bricks 0")


# ---- the work mask: runs of empty layers, flags on against flags off
_WORK = [(voxels, pose, ring) + SHAPES[(iv + ip + ir) % 3]
         for iv, voxels in enumerate(VOXELS) for ip, pose in enumerate(POSES) for ir, ring in enumerate(RINGS)]


@pytest.mark.parametrize("voxels,pose,ring,tile,shape", _WORK, ids=["%s-%s-ns%d-%d+%d" % (v, p, r, s[0], s[1]) for v, p, r, _, s in _WORK])
def test_work_mask_under_brick_flags(R, voxels, pose, ring, tile, shape):
    _push(R, _scene(voxels, 40, pose, "sparse"))
    g, s, s0, plan = _frames(R, tile, ring)
    _check_ring(plan, ring, shape)
    assert plan["bricks"] == 1, "the planner dropped the flags: no layer of bricks is empty"
    assert s[..., 3].max() > 0.05, "the frame shows nothing"
    _same(g, s, "against the gather kernel")
    _same(s, s0, "against the frame with bricks 0")


# ---- the nested block's variants
_TABLES = ("dense", "dense_h", "sparse_h", "dense3d")
_BLOCK = [(table, voxels, ring, POSES[(it + iv + ir) % 6]) + SHAPES[ish]
          for it, table in enumerate(_TABLES) for iv, voxels in enumerate(VOXELS) for ir, ring in enumerate(RINGS) for ish in range(3)]


@pytest.mark.parametrize("table,voxels,ring,pose,tile,shape", _BLOCK,
                         ids=["%s-%s-ns%d-%s-%d+%d" % (t, v, r, p, s[0], s[1]) for t, v, r, p, _, s in _BLOCK])
def test_visible_block_variants(R, table, voxels, ring, pose, tile, shape):
    _push(R, _scene(voxels, 40, pose, table))
    g, s, s0, plan = _frames(R, tile, ring)
    _check_ring(plan, ring, shape)
    if table == "dense3d":
        assert plan["fast_tf"] == 0, plan
    else:
        assert plan["fast_tf"] == 1 and plan["use_ah"] == (1 if table.endswith("_h") else 0), plan
    assert s[..., 3].max() > 0.05, "the frame shows nothing"
    _same(g, s, "against the gather kernel")
    _same(s, s0, "against the frame with bricks 0")


_EXTRA = [(voxels, ring, ("sparse", "dense3d", "sparse_h")[(iv + ir + ish) % 3], POSES[(2 * iv + ir + ish) % 6]) + SHAPES[ish]
          for iv, voxels in enumerate(VOXELS) for ir, ring in enumerate(RINGS) for ish in range(3)]
_EXTRA_IDS = ["%s-ns%d-%s-%s-%d+%d" % (v, r, t, p, s[0], s[1]) for v, r, t, p, _, s in _EXTRA]


@pytest.mark.parametrize("voxels,ring,table,pose,tile,shape", _EXTRA, ids=_EXTRA_IDS)
def test_first_hit_depth(R, voxels, ring, table, pose, tile, shape):
    _push(R, _scene(voxels, 40, pose, table))
    (g, gd), (s, sd), (s0, sd0), plan = _frames(R, tile, ring, depth=True)
    _check_ring(plan, ring, shape)
    _same(g, s, "against the gather kernel")
    _same(s, s0, "against the frame with bricks 0")
    fin = np.isfinite(gd)
    assert fin.any(), "no ray hit anything"
    for d, what in ((sd, "with flags"), (sd0, "with bricks 0")):
        assert np.array_equal(fin, np.isfinite(d)) and np.array_equal(gd[fin], d[fin]), "first-hit depth %s differs from the gather kernel's" % what


@pytest.mark.parametrize("voxels,ring,table,pose,tile,shape", _EXTRA, ids=_EXTRA_IDS)
def test_gl_max_blend(R, voxels, ring, table, pose, tile, shape):
    _push(R, _scene(voxels, 40, pose, table))
    g, s, s0, plan = _frames(R, tile, ring, blend=2)
    _check_ring(plan, ring, shape)
    assert s[..., 3].max() > 0.0, "the frame shows nothing"   # (the largest single alpha: a few percent under the dense tables)
    _same(g, s, "against the gather kernel")
    _same(s, s0, "against the frame with bricks 0")
