"""The column-stream kernel at every ring plan, DMA width and shape (tests/_cols_plan_cases.py has the cases, their data and
the classes; tests/_cols_plan_ref.py the planner's rules; tests/test_cols_plan_cpu.py qualifies both without a GPU).

Every case forces the column-stream kernel (option kernel 3 raises where it declines), reads the launch plan back
(smk_get_stat "cols_plan_*") and holds it to what the case was dialled to and to the rules -- a planner change that moves a
case out of its class fails here, with the new plan in the message.  The frame must be within 2e-5 of the gather kernel's
(the blend is re-associated per job: a few ulp per segment, and the cases keep a ray's non-empty segments few), bit-identical
under the MAX blend, within 1e-4 of the CPU checker, with no status word and no failure counted, and the kernel's sample
count must equal the checker's in-volume count: every sample exactly once, whatever the plan.

test_tally then asserts the coverage over the cases that ran: every class on every principal axis, in both marching
directions, at both workgroup shapes and for both voxel types (the table it prints is profiles/cols_plans.md).

Unreachable, left out of the tally (tests/_cols_plan_cases.py UNREACHABLE, proved by the CPU sweep): a cols_fly request
lowered by the n_ch * maxfly <= 63 rule at shape 2 -- two loaders share nslots - 2 slots, and the slices that fit LDS keep
n_ch * (nslots - 2) / 2 below 63.

A ray with more than 4095 planes inside one job (status 5): test_more_planes_than_a_list_entry_holds."""
import numpy as np
import pytest

import _cols_plan_ref as ref
import oracle
from _cols_plan_cases import (BY_NAME, CASES, KNOBS, REFUSED_CASE, build_scene, classes_of, expected_plan, tally)
from _scenes import push_scene

pytestmark = pytest.mark.gpu
TOL = 1e-4      # against the checker
TOL_G = 2e-5    # against the gather kernel (tests/test_gpu_cols.py)
RAN = []        # (case, plan) of every case that ran, for test_tally
PERM = {"z": 0, "y": 1, "x": 2}


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def read_plan(R):
    return {f: int(R.stat("cols_plan_" + f)) for f in ref.FIELDS}


def reset(R):
    for k in KNOBS:
        R.set_option(k, 0)
    R.set_option("cols_counts", 0)
    R.set_option("kernel", 0)
    R.set_blend(0)


def set_knobs(R, c, **more):
    opts = dict(c["opts"], cols_shape=c["shape"], **more)
    for k in KNOBS:
        R.set_option(k, opts.get(k, 0))


def render(R):
    """R.render(); a status word (a protocol time-out above all) or a HIP error is a finding to read from the code, not to
    run into again case after case: the module's run ends there.  A refusal is an ordinary failure"""
    try:
        return R.render()
    except Exception as e:
        if type(e).__name__ != "SmkError" or "not applicable" in str(e):
            raise
        pytest.exit("the sweep ends: %s" % e, returncode=3)


def both(R, blend=0):
    """the current frame set-up on the gather and the column-stream kernel"""
    R.set_blend(blend)
    R.set_option("kernel", 1)
    g = render(R)
    assert R.last_frame_info()[0] == 1
    R.set_option("kernel", 3)          # raises where the column-stream kernel declines the frame
    R.set_option("cols_counts", 1)
    s = render(R)
    assert R.last_frame_info()[0] == 4, "the frame was declined"
    return g, s


def check_plan(c, plan, jobs):
    wrong = []
    if plan["nslots"] < 3 or plan["n_ch"] < 1:
        return ["no plan was read back"]
    if c["one"] and (plan["cw"], plan["ch"], plan["ncu"], plan["ncv"]) != (c["nu"] - 1, c["nv"] - 1, 1, 1):
        wrong.append("the face is no longer one column of %d x %d cells: re-dial the case (tests/_cols_plan_cases.py)" % (c["nu"] - 1, c["nv"] - 1))
    try:
        rules = expected_plan(c, plan["cw"], plan["ch"], plan["dir"])
    except ref.Refused as e:
        return wrong + ["the rules refuse these columns: %s" % e]
    diff = {k: (rules[k], plan[k]) for k in plan if k in rules and rules[k] != plan[k]}
    if diff:
        wrong.append("the rules give another plan, (rules, read back): %r" % diff)
    if jobs != rules["jobs"]:
        wrong.append("cols_jobs is %d, the rules give %d" % (jobs, rules["jobs"]))
    if plan["perm"] != PERM[c["pose"][0]] or plan["dir"] not in (1, -1):
        wrong.append("perm %d dir %d under pose %s" % (plan["perm"], plan["dir"], c["pose"]))
    for k, v in c["want"].items():
        if plan[k] != v:
            wrong.append("%s is %d, dialled to %d" % (k, plan[k], v))
    left = set(c["cls"]) - classes_of(c, plan)
    if left:
        wrong.append("the case left the classes it was dialled to: %s" % ", ".join(sorted(left)))
    return wrong


def run_case(R, c):
    """renders the case on both kernels; returns (plan, list of what is wrong)"""
    wrong = []
    sc = build_scene(c)
    chk = sc.render()
    want_samples = oracle.inside_samples()      # (the checker marches every plane of every ray: no early termination)
    try:
        set_knobs(R, c)
        push_scene(R, sc)
        fails0 = R.stat("slab_failures")
        g, s = both(R)
        plan, jobs = read_plan(R), int(R.stat("cols_jobs"))
        samples, segments = R.stat("cols_samples"), R.stat("cols_segments")
        if R.stat("slab_status") != 0:
            wrong.append("slab_status %d" % R.stat("slab_status"))
        diff, err = float(np.abs(g - s).max()), float(np.abs(s - chk).max())
        print("%s: against the checker %.3g, against gather %.3g, alpha max %.3f, %d samples in %d segments of %d jobs; %s" %
              (c["name"], err, diff, s[..., 3].max(), samples, segments, jobs, " ".join("%s %d" % (k, plan[k]) for k in ref.FIELDS)))
        if diff > TOL_G:
            bad = np.argwhere(np.abs(g - s).max(-1) > TOL_G)[0]
            wrong.append("differs from the gather kernel by %g, first at pixel (%d, %d)" % (diff, bad[1], bad[0]))
        if err > TOL:
            wrong.append("differs from the checker by %g" % err)
        if not s[..., 3].max() > 0.05:
            wrong.append("the frame shows nothing (alpha max %g)" % s[..., 3].max())
        if s[..., 3].max() >= 1.0:
            wrong.append("a ray saturates: the sample count would not be the checker's")
        if samples != want_samples:
            wrong.append("cols_samples %d, the checker counts %d in-volume samples" % (samples, want_samples))
        if not segments > 0:
            wrong.append("no segment was written")
        if c["ends"]:       # both slabs show: the keys of the first and of the last chunks are both in the frame
            for keep in ((True, False), (False, True)):
                one = build_scene(c, keep).render()
                if not np.abs(one - chk).max() > 1e-3:
                    wrong.append("the frame is that of one end slab alone %r: vacuous" % (keep,))
        mg, ms = both(R, 2)
        if not np.array_equal(mg, ms):
            wrong.append("MAX blend differs from the gather kernel by %g" % np.abs(mg - ms).max())
        if R.stat("slab_status") != 0:
            wrong.append("slab_status %d under the MAX blend" % R.stat("slab_status"))
        if R.stat("slab_failures") != fails0:
            wrong.append("slab_failures moved by %g" % (R.stat("slab_failures") - fails0))
        if read_plan(R) != plan:
            wrong.append("the MAX-blend frame got another plan")
    finally:
        reset(R)
    return plan, jobs, wrong


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case(R, c):
    plan, jobs, wrong = run_case(R, c)
    RAN.append((c, plan))
    wrong += check_plan(c, plan, jobs)
    assert not wrong, "%s: %s\nplan: %r" % (c["name"], "; ".join(wrong), plan)


def test_clamp_shows_in_the_read_back(R):
    """the asked band wait is above, the planned one at, nslots - 2"""
    for name, asked in (("wstep-clamp-ns3-a", 3), ("wstep-clamp-ns4-b", 6)):
        c = BY_NAME[name]
        assert c["opts"]["cols_wstep"] - 1 == asked
        try:
            set_knobs(R, c)
            push_scene(R, build_scene(c))
            both(R)
            p = read_plan(R)
            assert asked > p["nslots"] - 2 == p["wstep"] and p["nslots"] == c["opts"]["cols_ns"], p
            assert R.stat("slab_status") == 0
        finally:
            reset(R)


# ------------------------------------------------------------------------------------------------ knob invariance
# Segments depend only on the columns and the chunks: frames whose plans agree in (cw, ch, cl, nck) must agree bit for bit,
# whatever the ring does.  A difference is a protocol error -- a slot overwritten early or read late.
_INV = {"cols_ns": (0, 3, 5), "cols_fly": (0, 1, 4), "cols_wstep": (0, 1, 7), "cols_take_min": (0, 1, 64), "cols_take_wait": (0, 50),
        "cols_shape": (1, 2)}
_INV_BASES = {
    # several columns, three chunks, f32, S = z; one long u8 column, S = y
    "columns-and-chunks": dict(name="inv-columns", pose="z+", nu=42, nv=30, ns=24, dims=(42, 30, 24), f32=True, shape=1, size=(64, 64), steps=40,
                               opts={"cols_chunk": 8}, ends=0.0, fill=0.9, depth=0.4, one=False),
    "long-column-u8": dict(name="inv-long", pose="y-", nu=24, nv=10, ns=60, dims=(24, 60, 10), f32=False, shape=2, size=(20, 20), steps=90,
                           opts={}, ends=0.0, fill=0.8, depth=0.4, one=True),
}


@pytest.mark.parametrize("which", sorted(_INV_BASES))
def test_frames_do_not_depend_on_the_ring(R, which):
    import itertools
    c = _INV_BASES[which]
    sc = build_scene(c)
    chk = sc.render()
    groups = {}
    try:
        push_scene(R, sc)
        R.set_option("kernel", 3)
        R.set_option("cols_chunk", c["opts"].get("cols_chunk", 0))
        names = sorted(_INV)
        for combo in itertools.product(*(_INV[k] for k in names)):
            for k, v in zip(names, combo):
                R.set_option(k, v)
            f = render(R)
            assert R.last_frame_info()[0] == 4 and R.stat("slab_status") == 0, combo
            p = read_plan(R)
            key = (p["cw"], p["ch"], p["cl"], p["nck"])
            if key not in groups:
                assert np.abs(f - chk).max() <= TOL and f[..., 3].max() > 0.05, (combo, key)
                groups[key] = (f, combo, 1, {(p["nslots"], p["maxfly"], p["wstep"], p["shape"])})
            else:
                first, combo0, n, rings = groups[key]
                assert np.array_equal(first, f), "knobs %r and %r (%r) give the columns %r and frames that differ by %g" % (
                    combo0, combo, names, key, np.abs(first - f).max())
                rings.add((p["nslots"], p["maxfly"], p["wstep"], p["shape"]))
                groups[key] = (first, combo0, n + 1, rings)
        print("%s: %s" % (which, {k: (v[2], len(v[3])) for k, v in groups.items()}))
        assert max(len(v[3]) for v in groups.values()) >= 8 and sum(v[2] for v in groups.values()) == 324, "the knobs did not move the ring"
    finally:
        reset(R)


# ------------------------------------------------------------------------------------------------ mask words across frames
def test_mask_words_across_frames(R):
    """the resolve pass clears what it reads: frames with two, one and two mask words again on one context and window each
    equal their first rendering"""
    c = BY_NAME["keys70-a"]
    try:
        push_scene(R, build_scene(c))
        R.set_option("kernel", 3)
        R.set_option("cols_shape", c["shape"])
        first = {}
        for chunk, words in ((4, 2), (0, 1), (4, 2), (256, 1), (0, 1), (4, 2)):
            R.set_option("cols_chunk", chunk)
            f = render(R)
            assert R.stat("cols_plan_mask_words") == words and R.stat("slab_status") == 0
            assert f[..., 3].max() > 0.05
            if chunk in first:
                assert np.array_equal(first[chunk], f), "cols_chunk %d: the frame changed by %g" % (chunk, np.abs(first[chunk] - f).max())
            first.setdefault(chunk, f)
    finally:
        reset(R)


# ------------------------------------------------------------------------------------------------ refusals and limits
def test_more_than_512_segment_keys_are_refused(R, smk):
    c = REFUSED_CASE
    try:
        set_knobs(R, c)
        push_scene(R, build_scene(c))
        R.set_option("kernel", 3)
        with pytest.raises(smk.SmkError) as e:
            R.render()
        assert str(e.value).endswith("not applicable: " + c["refused"]), str(e.value)
    finally:
        reset(R)


def _planes_inside(sc, dims):
    """per pixel, the planes of its ray whose sample lies inside the volume's box [-0.5, N - 0.5]^3 (float64: a count, the
    margin below covers the rounding), and |B| along each axis"""
    rc = sc.raycoef()
    i, j = np.meshgrid(np.arange(sc.width), np.arange(sc.height))
    px, py = (i + 0.5) * rc.pxs + rc.pxl, (j + 0.5) * rc.pys + rc.pyl
    m = np.arange(rc.nplanes, dtype=np.float64)[:, None, None]
    inside = np.ones((rc.nplanes,) + px.shape, bool)
    B = []
    for a in range(3):
        Aa, Ba = px * rc.Ax[a] + py * rc.Ay[a] + rc.Ac[a], px * rc.Bx[a] + py * rc.By[a] + rc.Bc[a]
        p = Aa + m * Ba
        inside &= (p >= -0.5) & (p <= dims[a] - 0.5)
        B.append(np.abs(Ba))
    return inside.sum(0), B


def test_more_planes_than_a_list_entry_holds(R, smk):
    """A listed ray carries its plane count in 12 bits: a job in which some ray has more than 4095 planes reports status 5
    and the forced frame fails with that text.  6 x 6 x 41 voxels under 5200 planes: in one chunk of 40 positions the
    longest ray has about 4600 planes inside; in chunks of 4 positions (cols_chunk 4) a job holds 4 slices, 5.5 where it
    takes the volume's half voxels, of a ray's 41: at most (5.5 / |B_s|) + 2 planes, about 620 -- both computed from the
    case's ray coefficients below before either frame is relied on.  Material sits in the two end slabs only (as in the
    sweep's long cases), so the frame in chunks keeps few non-empty segments per ray and the 2e-5 bound applies (measured:
    6e-7 off the gather kernel and off the checker, alpha up to 0.998)"""
    from _slab_plan_cases import model_dims
    c = dict(BY_NAME["dma1-full-a"], name="planes-5200", nu=6, nv=6, ns=41, steps=5200, opts={}, ends=0.05)
    c["dims"] = model_dims(c["pose"], 6, 6, 41)
    sc = build_scene(c)
    count, B = _planes_inside(sc, c["dims"])
    bs = B[{"z": 2, "y": 1, "x": 0}[c["pose"][0]]]
    assert count.max() > 4095 + 8, count.max()
    assert (5.5 / bs.min()) + 2 < 4095 - 8, 5.5 / bs.min()
    chk = sc.render()
    try:
        set_knobs(R, c)
        push_scene(R, sc)
        fails0 = R.stat("slab_failures")
        R.set_option("kernel", 3)
        with pytest.raises(smk.SmkError) as e:
            R.render()
        assert "the column-stream kernel reported a ray it cannot list (status 5" in str(e.value), str(e.value)
        assert R.stat("slab_failures") == fails0 + 1
        assert R.stat("cols_plan_nck") == 1 and R.stat("cols_plan_cl") == 40
        R.set_option("cols_chunk", 4)
        g, s = both(R)
        assert R.stat("cols_plan_nck") == 10 and R.stat("slab_status") == 0 and R.stat("slab_failures") == fails0 + 1
        print("planes-5200 in chunks of 4: against the checker %.3g, against gather %.3g, alpha max %.3f" %
              (np.abs(s - chk).max(), np.abs(g - s).max(), s[..., 3].max()))
        assert s[..., 3].max() > 0.05
        assert np.abs(g - s).max() <= TOL_G and np.abs(s - chk).max() <= TOL
    finally:
        reset(R)


def test_plan_stats_read_zero_after_another_kernel(R):
    c = CASES[0]
    try:
        set_knobs(R, c)
        push_scene(R, build_scene(c))
        both(R)
        assert R.stat("cols_plan_n_ch") > 0 and R.stat("cols_plan_nslots") >= 3
        R.set_option("kernel", 1)
        R.render()
        assert R.last_frame_info()[0] == 1
        assert all(R.stat("cols_plan_" + f) == 0 for f in ref.FIELDS)
    finally:
        reset(R)


# ------------------------------------------------------------------------------------------------ shards
def test_columns_and_chunks_on_two_shards(gpu_renderer_factory):
    """several columns and chunks on both ranks of a two-rank shard -- the second rank's stored box has a non-zero origin,
    both have a halo -- merged as tests/test_gpu_layouts.py merges them and held to the checker's unsharded frame, each rank
    to the checker's frame of its region"""
    import torch
    from simian_spacemonkey_amd import sortlast
    c = _INV_BASES["columns-and-chunks"]
    sc = build_scene(c)
    chk = sc.render()
    world, npix = 2, sc.width * sc.height
    regions = [sortlast.shard_region(sc.dims, r, world) for r in range(world)]
    assert any(any(o != 0 for o in reg[0]) for reg in regions)
    layers = torch.zeros((world, npix, 4), dtype=torch.float32, device="cuda")
    rs = []
    try:
        for r in range(world):
            Rr = gpu_renderer_factory()
            rs.append(Rr)
            Rr.set_shard(r, world)
            push_scene(Rr, sc)
            Rr.set_option("cols_chunk", 4)
            Rr.set_option("cols_shape", 1 + r)
            Rr.set_option("kernel", 3)
            Rr.render_device(layers[r].data_ptr(), None, None)
        torch.cuda.synchronize()
        for Rr in rs:
            assert Rr.last_frame_info()[0] == 4
            assert Rr.stat("slab_status") == 0 and Rr.stat("slab_failures") == 0
            p = read_plan(Rr)
            assert p["ncu"] * p["ncv"] > 1 and p["nck"] > 1, p
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        rs[0].composite_over_device(layers.data_ptr(), world, rs[0].shard_order(world), npix, out.data_ptr(), None)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(sc.height, sc.width, 4)
        assert chk[..., 3].max() > 0.05 and np.abs(got - chk).max() <= TOL, np.abs(got - chk).max()
        for r in range(world):
            part = build_scene(c)
            part.region = regions[r]
            pr = part.render()
            e = np.abs(layers[r].cpu().numpy().reshape(sc.height, sc.width, 4) - pr).max()
            assert pr[..., 3].max() > 0.05 and e <= TOL, (r, e)
    finally:
        for Rr in rs:
            Rr.close()


def test_tally():
    """the coverage the sweep is for, over the cases that ran: none skipped, none left out"""
    assert [c["name"] for c, _ in RAN] == [c["name"] for c in CASES], "the tally needs every case of this module to have run"
    rows, missing = tally(RAN)
    print("| class | cases | bases | covers |\n|---|---|---|---|\n" + "\n".join(rows))
    assert not missing, "not reached: %s" % "; ".join(missing)
