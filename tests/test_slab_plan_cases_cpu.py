"""The plan sweep's data and cases held to their purpose with the CPU checker alone (tests/_slab_plan_cases.py; the sweep
itself is tests/test_gpu_slab_plans.py).  No GPU."""
import numpy as np
import pytest

from _slab_plan_cases import BY_NAME, CASES, PLANS, build_scene, corner_drift, noise_volume, table2d, tally

BAR = 1e-3     # ten times the GPU suite's tolerance against the checker: a wrong voxel cannot hide under it
# a thin u8 slab on a narrow pitch, an f32 volume on a wide one, and a stick of 70 slices (the deepest voxels weigh least): the
# dense table's alpha (dense_alpha: about one optical depth over the case's planes, whatever their number) was chosen so
# that the bar holds for these.  All three have a pixel and a plane for every two voxels or better; a case that samples its
# volume more coarsely on purpose (stick-200: 60 planes for 200 slices, for a deep band) cannot show a voxel no sample touches.
REPRESENTATIVE = ["p24-u8-g3", "p40-f32-g3", "stick-fly3"]


@pytest.mark.parametrize("name", REPRESENTATIVE)
def test_one_wrong_voxel_moves_the_frame(name):
    """any one of 16 seeded voxels replaced by its complement moves the checker's frame by more than 1e-3"""
    c = BY_NAME[name]
    v8, vf, nrm = noise_volume(c)
    base = build_scene(c, (v8, vf, nrm)).render()
    assert base[..., 3].max() > 0.05
    rng = np.random.default_rng(1234)
    nz, ny, nx = v8.shape[:3]
    moved = []
    for _ in range(16):
        z, y, x = int(rng.integers(nz)), int(rng.integers(ny)), int(rng.integers(nx))
        w8, wf = v8.copy(), vf.copy()
        w8[z, y, x] = 255 - w8[z, y, x]
        wf[z, y, x] = np.float32(1.0) - wf[z, y, x]
        frame = build_scene(c, (w8, wf, nrm)).render()       # (the normals stay: only the voxel's own 8 or 16 bytes change)
        moved.append(float(np.abs(frame - base).max()))
    print(name, "smallest move %.3g, largest %.3g" % (min(moved), max(moved)))
    assert min(moved) > BAR, moved


def test_the_generator_keeps_its_promises():
    for c in CASES:
        v8, vf, _ = noise_volume(c)
        w8, wf, _ = noise_volume(c)
        assert np.array_equal(v8, w8) and np.array_equal(vf, wf)               # seeded by the case alone
        assert v8.shape[:3] == tuple(reversed(c["dims"])) and min(c["dims"]) >= 2 and max(c["nu"], c["nv"]) <= 66 and c["ns"] <= 200
        if c["table"] in ("dense", "dense_h"):
            t = table2d(c, False)
            assert t[..., 3].min() >= 2 and t[..., 3].max() <= 80               # every texel contributes, none is opaque
        elif c["table"].startswith("sparse"):
            t = table2d(c, True)
            clear = (t[..., 3] == 0)
            assert 0.2 < clear.mean() < 0.6 and clear.all(axis=0).any() and clear.all(axis=1).any()   # whole bands of values and of gradients
    # neighbours differ (as whole voxels) in the noise: spot-check one case along every axis
    v8, vf, _ = noise_volume(BY_NAME["p40-f32-g3"])
    for ax in range(3):
        assert (np.diff(v8.astype(np.int32), axis=ax) != 0).any(-1).all() and (np.diff(vf, axis=ax) != 0).any(-1).all()


def test_dense_frames_never_saturate():
    """under the dense table no ray of the checker's frame reaches alpha 1: the loaders stream every slice"""
    for c in CASES:
        if c["table"] == "dense" and c["feature"] is None:
            f = build_scene(c).render()
            assert 0.05 < f[..., 3].max() < 1.0, c["name"]


def test_the_recorded_plans_meet_the_tally():
    """the plans the cases were dialled to (PLANS) reach everything the sweep's tally asks for, and the close-up's corner
    rays drift more than 2 voxels per slice -- so a tally that fails on the GPU says the planner moved, not the cases"""
    assert sorted(PLANS) == sorted(BY_NAME)
    recs = []
    for c in CASES:
        p = dict(PLANS[c["name"]])
        if c["name"] == "closeup":
            p["drift"] = corner_drift(build_scene(c), p["perm"])
            assert 2.0 < p["drift"] < 3.0
        recs.append((c, p))
    rows, missing = tally(recs)
    assert not missing, missing
