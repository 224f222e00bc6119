"""The consumer loop of the slice-ring kernel after its instruction diet (*Instruction stream of a
turn*): scalar fp32 where the compiler paired the two channels' lerps, the slice-table entry by one multiply-add, every
later batch of corner reads through the first batch's four addresses and the instruction's offset field, the texel offset
by a 24-bit multiply.  None of it may change a bit of a frame.

The reference is the gather kernel (option kernel 1), which shares none of the edited code.  Every slice-ring frame (option
kernel 2: a declined frame raises, nothing falls back) must equal it bit for bit, with no status word, failure or retry.

Shapes: a 48^3 volume of per-voxel noise with normals (the generator of tests/test_gpu_slab_plans.py, seeded by the case
name) at 96 x 96 pixels and 96 planes -- several tiles, several waves a tile, more slices than a ring holds; every texel,
table entry and corner address of a wrong place holds other numbers than the right one.
  * f32, u8 and u16 voxels; the three principal axes, both marching directions;
  * R8k shading under the 2-D table without and with the third-axis alpha and under the dense 3-D table; the 1-D colour
    table unshaded;
  * brick flags on and off; a table with clear bands over a volume whose middle third lies inside them, so that whole
    layers of bricks come out empty and rays step over runs of them (test_runs_of_empty_layers_are_stepped_over holds the
    diagnostic instance's counters to that), and the reference's dense default ramp, under which every sample takes the
    visible path;
  * first-hit depth; the 12 + 4-wave and the 8 + 2-wave workgroups beside the 10 + 2 ones (option tile)."""
import functools
import os

import numpy as np
import pytest

import oracle as O
import _u16_ref as U
from _scenes import push_scene
from _slab_plan_cases import build_scene, case, noise_volume

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOXELS = ("f32", "u8", "u16")
POSES = ("z+", "z-", "y+", "y-", "x+", "x-")
# (table, brick flags): "sparse" has the clear bands, "ramp" is the dense default ramp, "_h" adds the third-axis alpha
TABLES = (("sparse", 0), ("sparse", 1), ("sparse_h", 1), ("ramp", 0), ("ramp", 1), ("dense3d", 0), ("dense3d", 1), ("1d", 1))
KNOBS = (("kernel", 0), ("bricks", 1), ("tile", 0), ("lockstep", 1))


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


@functools.lru_cache(maxsize=None)
def _volume(pose):
    """(u8 VGH, f32 VGH, normals) of the pose's case: the middle third of the slices along its marching axis holds values
    inside the sparse table's clear band"""
    v8, vf, nrm = noise_volume(_case(pose, "sparse"))
    for a in (v8, vf, nrm):
        a.setflags(write=False)
    return v8, vf, nrm


def _case(pose, table):
    kind = {"ramp": "dense", "1d": "dense"}.get(table, table)
    return case("diet-" + pose, pose, 48, 48, 48, table=kind, hole=True, size=(96, 96), steps=96, fill=0.9, depth=0.9,
                shade=0 if table == "1d" else 1)


@functools.lru_cache(maxsize=None)
def _scene(voxels, pose, table):
    """what push() needs of the case: the checker's scene object carries the frame state, nothing is rendered on the CPU"""
    c = _case(pose, table)
    v8, vf, nrm = _volume(pose)
    vol16 = None
    if voxels == "u16":   # the same noise as 16-bit integers; the scene holds their decoded values
        vol16 = np.ascontiguousarray((vf.astype(np.float64) * 65535.0).astype(np.uint16))
        vf = U.decode_u16(vol16)
    sc = build_scene(dict(c, f32=voxels != "u8"), volume=(v8, vf, nrm))
    if table == "ramp":
        sc.tf_vg = np.load(os.path.join(GOLDEN, "tf_cfg2_deptex.npy"))
    if table == "1d":     # one channel under the 1-D colour table (premultiplied on upload), unshaded
        data = sc.data[..., :1]
        sc1 = O.Scene(np.ascontiguousarray(data), fsize=tuple(sc.fsize))
        for k in ("width", "height", "steps", "xform", "frustum"):
            setattr(sc1, k, getattr(sc, k))
        sc1.tf_mode, sc1.tlut, sc1.shade_mode = 0, U.table_1d(), 0
        sc = sc1
        if vol16 is not None:
            vol16 = np.ascontiguousarray(vol16[..., :1])
    if vol16 is not None:
        sc.dmode = "V1" if table == "1d" else "VGH"
        return U.Case(vol16, sc)
    return sc


def _push(R, s):
    if isinstance(s, U.Case):
        U.push(R, s)
    else:
        push_scene(R, s)


def _both(R, bricks=1, tile=0, **kw):
    """the frame on the gather kernel and on the forced slice-ring kernel"""
    fails0, retries0 = R.stat("slab_failures"), R.stat("slab_retries")
    R.set_option("bricks", bricks)
    R.set_option("kernel", 1)
    g = R.render(**kw)
    assert R.last_frame_info()[0] == 1
    R.set_option("kernel", 2)
    R.set_option("tile", tile)
    s = R.render(**kw)
    assert R.last_frame_info()[0] == 2, "the frame was declined"
    assert R.stat("slab_status") == 0
    assert R.stat("slab_failures") == fails0 and R.stat("slab_retries") == retries0
    return g, s


@pytest.mark.parametrize("table,bricks", TABLES, ids=["%s-b%d" % t for t in TABLES])
@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("voxels", VOXELS)
def test_frame_equals_the_gather_kernel(R, voxels, pose, table, bricks):
    _push(R, _scene(voxels, pose, table))
    g, s = _both(R, bricks)
    assert s[..., 3].max() > 0.05, "the frame shows nothing"
    assert np.array_equal(g, s), "differs from the gather kernel by %g in %d pixels" % (np.abs(g - s).max(), (g != s).any(-1).sum())


def test_runs_of_empty_layers_are_stepped_over(R):
    """the diagnostic instance (float voxels, R8k, 2-D table, brick-flag code) counts its lanes: with the flags on, fewer
    lanes interpolate a sample than there are samples inside the volume (the count with the flags off), and fewer lanes
    take a turn at all -- the planes of a run of empty layers are never visited"""
    _push(R, _scene("f32", "z+", "sparse"))
    R.set_option("lockstep", 1 | 16)
    g, off = _both(R, 0)
    in_volume, turns_off = R.stat("slab_inside_lanes"), R.stat("slab_active_lanes")
    _, on = _both(R, 1)
    inside, turns_on = R.stat("slab_inside_lanes"), R.stat("slab_active_lanes")
    assert R.stat("slab_plan_bricks") == 1, "the planner dropped the flags: no layer of bricks is empty"
    assert np.array_equal(g, off) and np.array_equal(g, on)
    assert in_volume > 0 and in_volume == turns_off, (in_volume, turns_off)
    assert inside < in_volume, (inside, in_volume)
    assert turns_on < turns_off, (turns_on, turns_off)


@pytest.mark.parametrize("voxels", VOXELS)
def test_first_hit_depth(R, voxels):
    _push(R, _scene(voxels, "y-", "sparse"))
    (g, gd), (s, sd) = _both(R, 1, depth=True)
    assert np.array_equal(g, s)
    fin = np.isfinite(gd)
    assert fin.any() and np.array_equal(fin, np.isfinite(sd)) and np.array_equal(gd[fin], sd[fin])


@pytest.mark.parametrize("table", ["sparse_h", "ramp", "dense3d"])
@pytest.mark.parametrize("voxels", VOXELS)
def test_every_workgroup_shape(R, voxels, table):
    """the planner's own choice at this size, the 12 + 4-wave shape (tile 4) and the 8 + 2-wave one (tile 5): between them
    all three shapes of the loop"""
    _push(R, _scene(voxels, "x+", table))
    shapes = set()
    for tile in (0, 4, 5):
        g, s = _both(R, 1, tile)
        shapes.add((int(R.stat("slab_plan_nw")), int(R.stat("slab_plan_nl"))))
        assert np.array_equal(g, s), "tile %d: differs from the gather kernel by %g" % (tile, np.abs(g - s).max())
        R.set_option("tile", 0)
    assert shapes == {(10, 2), (12, 4), (8, 2)}, shapes
