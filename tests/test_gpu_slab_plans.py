"""The slice-ring kernel at every window pitch and ring plan (tests/_slab_plan_cases.py has the cases and their data).

Every case forces the slice-ring kernel (option kernel 2 raises where it declines), reads the launch plan back
(smk_get_stat "slab_plan_*") and holds it to the plan the case was dialled to -- a planner change that moves a case out of
its class fails here, with the new plan in the message, and the case has to be dialled again -- and to the window-pitch rule
as tests/_slab_plan_ref.py restates it.  The frame must be bit-identical to the gather kernel's (colour, first-hit depth
where asked), also under the MAX blend, within 1e-4 of the CPU checker, with no status word, failure or retry.  Two cases
re-associate the blend by design and are held to the project's 2e-5 instead (tests/test_gpu_slab.py): the back-to-front
frame, which the kernel composites front to back, and the frame cut into three depth segments (slab_split 3), whose partial
frames are merged afterwards; their MAX-blend frames are bit-identical like everybody's.

test_tally then asserts the coverage over the cases that ran (the table it prints is the record of what the sweep reaches).

Classes the planner cannot reach, left out of the tally:
  * pitch 64 with ONE row group: rpg = 64 / gcd(64, 64) = 1 row, and slab_window declines windows of fewer than two rows
    ("degenerate window"; slab_refusal declines volumes thinner than two voxels), so groups = ceil(wv / 1) >= 2.
The window-pitch rule emits one class DESIGN.md does not name, pitch 4 (per 1, rpg 16: windows of at most 4 units and more
than 8 rows); the sweep covers it like the others.

The largest mych (DMA instructions of one loader per slice) the LDS allows: a ring needs 3 slots of chunks KiB beside the
slice table in 158 KiB (slab_ring), so chunks <= 52.  Small workgroups (a loader takes whole slices: mych = chunks): 52,
reached with 52 rows on pitch 64.  Big ones (two loaders share a slice's groups: mych = ceil(groups / 2) * per with
groups * per <= 52): 28 = 4 * 7, reached with 7 groups on pitch 56 (per 3: 9 * 3 = 27, per 5: 5 * 5 = 25, per 1: 26)."""
import numpy as np
import pytest

import _slab_plan_ref as ref
from _scenes import push_scene
from _slab_plan_cases import CASES, PLAN_FIELDS, PLANS, build_scene, corner_drift, stored_extents, tally

pytestmark = pytest.mark.gpu
TOL = 1e-4          # against the checker
TOL_REASSOC = 2e-5  # against the gather kernel where the blend is re-associated
KNOBS = {"tile": 0, "slab_ns": 0, "slab_fly": 0, "slab_T": 0, "slab_split": 0, "bricks": 1, "kernel": 0}
RAN = []            # (case, plan) of every case that ran, for test_tally


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def read_plan(R):
    return {f: int(R.stat("slab_plan_" + f)) for f in PLAN_FIELDS}


def _checker(sc, c, blend, R):
    """the checker's frame (and first-hit depth) of the case, and the scene depth an occluded case renders under"""
    if c["feature"] == "shadows":
        return sc.render_shadow()[0], None, None
    if c["feature"] == "occluded":   # a fronto-parallel occluder midway between two planes = the free clip plane (0, 0, 1, d)
        rc = R.raycoef()
        d = float((rc.tau0 + (rc.nplanes // 2 + 0.5) * rc.dtau) * sc.znear)
        sc.clip_plane = (0.0, 0.0, 1.0, d)
        try:
            return sc.render(blend=blend), None, np.full((sc.height, sc.width), d, np.float32)
        finally:
            sc.clip_plane = None
    if c["feature"] == "depth":
        f, fd = sc.render(blend=blend, depth=True)
        return f, fd, None
    return sc.render(blend=blend), None, None


def run_case(R, c):
    """renders the case on both kernels; returns (plan, list of what is wrong)"""
    wrong = []
    sc = build_scene(c)
    depth = c["feature"] == "depth"
    try:
        for k, v in c["opts"].items():
            R.set_option(k, v)
        R.set_option("tile", c["tile"])
        push_scene(R, sc)
        R.set_blend(c["blend"])
        ref_rgba, ref_depth, zs = _checker(sc, c, c["blend"], R)
        kw = dict(depth=depth, scene_depth=zs) if zs is not None else dict(depth=depth)
        fails0, retries0 = R.stat("slab_failures"), R.stat("slab_retries")

        def both(blend):
            R.set_blend(blend)
            R.set_option("kernel", 1)
            g = R.render(**kw)
            assert R.last_frame_info()[0] == 1
            R.set_option("kernel", 2)          # raises where the slice-ring kernel declines the frame
            s = R.render(**kw)
            assert R.last_frame_info()[0] == 2, "the frame was declined"
            return (g, s) if depth else ((g, None), (s, None))

        (ga, gd), (sa, sd) = both(c["blend"])
        plan = read_plan(R)
        if R.stat("slab_status") != 0:
            wrong.append("slab_status %d" % R.stat("slab_status"))
        reassoc = c["blend"] == 1 or c["opts"].get("slab_split", 0) >= 2
        diff = float(np.abs(ga - sa).max())
        if (diff > TOL_REASSOC) if reassoc else not np.array_equal(ga, sa):
            wrong.append("differs from the gather kernel by %g (%d pixels)" % (diff, int((ga != sa).any(-1).sum())))
        if depth:
            fin = np.isfinite(gd)
            if not (np.array_equal(fin, np.isfinite(sd)) and np.array_equal(gd[fin], sd[fin])):
                wrong.append("first-hit depth differs from the gather kernel's")
            if not (np.array_equal(fin, np.isfinite(ref_depth)) and fin.any() and np.abs(ref_depth[fin] - sd[fin]).max() <= 1e-4):
                wrong.append("first-hit depth differs from the checker's")
        err = float(np.abs(sa - ref_rgba).max())
        print("%s: max abs err against the checker %.3g, against gather %.3g, alpha max %.3f" % (c["name"], err, diff, sa[..., 3].max()))
        if err > TOL:
            wrong.append("differs from the checker by %g" % err)
        if not sa[..., 3].max() > 0.05:
            wrong.append("the frame shows nothing (alpha max %g)" % sa[..., 3].max())
        (ma, _), (ms, _) = both(2)
        if not np.array_equal(ma, ms):
            wrong.append("MAX blend differs from the gather kernel by %g" % np.abs(ma - ms).max())
        if R.stat("slab_status") != 0:
            wrong.append("slab_status %d under the MAX blend" % R.stat("slab_status"))
        if R.stat("slab_failures") != fails0 or R.stat("slab_retries") != retries0:
            wrong.append("slab_failures / slab_retries moved: %g / %g" % (R.stat("slab_failures") - fails0, R.stat("slab_retries") - retries0))
        if read_plan(R) != plan:
            wrong.append("the MAX-blend frame got another plan")
        if c["name"] == "closeup":
            plan["drift"] = corner_drift(sc, plan["perm"])
    finally:
        for k, v in KNOBS.items():
            R.set_option(k, v)
        R.set_blend(0)
        R.set_shadow(0)
    return plan, wrong


def check_plan(c, plan):
    wrong = []
    # the stats read 0 after a frame of another kernel: run_case's last frame was the slice-ring kernel's, so non-zero here
    if plan["nslots"] < 3 or plan["chunks"] < 1:
        wrong.append("no plan was read back")
    big = plan["nw"] + plan["nl"] > 12
    Dv = stored_extents(c, plan["perm"])[1]
    ok, tried = ref.check_readback(plan["wu"], plan["wv"], big, Dv, plan)
    if not ok:
        wrong.append("window %d x %d: the rule gives %r" % (plan["wu"], plan["wv"], tried))
    want = PLANS.get(c["name"])
    got = {k: v for k, v in plan.items() if k not in ("lds_bytes", "drift")}
    if want is None:
        wrong.append("no recorded plan for this case; it got %r" % got)
    elif got != want:
        wrong.append("the case left the plan class it was dialled to: re-dial it (tests/_slab_plan_cases.py).  Changed: %r" %
                     {k: (want.get(k), got.get(k)) for k in got if want.get(k) != got.get(k)})
    for k, v in c.get("want", {}).items():
        if plan[k] != v:
            wrong.append("%s is %d, meant to be %d" % (k, plan[k], v))
    return wrong


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case(R, c):
    plan, wrong = run_case(R, c)
    RAN.append((c, plan))
    wrong += check_plan(c, plan)
    assert not wrong, "%s: %s\nplan: %r" % (c["name"], "; ".join(wrong), plan)


def test_plan_stats_read_zero_after_another_kernel(R):
    c = CASES[0]
    sc = build_scene(c)
    push_scene(R, sc)
    try:
        R.set_option("kernel", 2)
        R.render()
        assert R.stat("slab_plan_wp") > 0 and R.stat("slab_plan_nslots") >= 3
        R.set_option("kernel", 1)
        R.render()
        assert R.last_frame_info()[0] == 1
        assert all(R.stat("slab_plan_" + f) == 0 for f in PLAN_FIELDS)
    finally:
        R.set_option("kernel", 0)


def test_tally():
    """the coverage the issue asks for, over the cases that ran: none skipped, none left out"""
    assert [c["name"] for c, _ in RAN] == [c["name"] for c in CASES], "the tally needs every case of this module to have run"
    rows, missing = tally(RAN)
    print("\n".join(rows))
    assert not missing, "not reached: %s" % "; ".join(missing)
