"""The feature fuzz: the seeded random frames of tests/_fuzz_features.py -- every classification, voxel type, shading,
blend mode, first-hit depth, orthogonal clip / free clip plane / sub-box / shard, perturbation, on small ragged volumes under
close-up, panned and asymmetric views -- through all three ray-marchers, one test per case and kernel:

  test_gather        kernel = 1 against the CPU checker (1e-4; the depth rule of test_gpu_occlusion.py)
  test_slice_ring    kernel = 2: refused for perturbation, else taken or declined for a reason of geometry; a taken frame is
                     the gather kernel's bit for bit (2e-5 for a back-to-front frame, which it composites front to back),
                     its depth the same numbers, the same RGBA with and without the depth request, status word 0
  test_column_stream kernel = 3: refused for exactly the mode the case's features predict, else taken or declined for a
                     reason of geometry; a taken frame within 2e-5 of the gather kernel's (bit for bit under GL_MAX); every
                     fourth taken case is rendered again in another window without a new upload (the layout-reuse path)
  test_tally         each streaming kernel took at least half of the cases it takes by mode

tests/test_fuzz_features_cpu.py proves on the CPU that the generator covers the features and their products and that its
frames show something.  SMK_FUZZ_CASES / SMK_FUZZ_SEED widen the run by hand; tools/fuzz_one.py --features SEED CASE re-runs
a case with the worst pixels printed."""
import contextlib

import numpy as np
import pytest

import _fuzz_features as F
from _scenes import push_scene
from _shadow_pert_ref import region_extents
from test_gpu_occlusion import _depth_rule

pytestmark = pytest.mark.gpu
TOL = 1e-4        # against the CPU checker: the suite's tolerance
TOL_G = 2e-5      # re-associated blends against the gather kernel (test_gpu_cols.py, test_gpu_slab.py)
NCASES, SEED = F.NCASES, F.SEED

# what the planners may answer for a view they cannot stream -- geometry, never a mode, memory or a missing instance
SLAB_GEOMETRIC = {
    "rays do not share a marching direction",
    "view too oblique for the principal axis",
    "degenerate window",
    "slice table does not fit LDS",
    "no configuration fits",
}
COLS_GEOMETRIC = {
    "rays do not share a marching direction",
    "view too oblique for the principal axis",
    "degenerate projection",
    "volume centre behind the eye",
    "volume reaches behind the eye",
    "no column size fits the lanes (view too close)",
}
COLS_MODES = (("pert", "perturbation"), ("btf", "back-to-front blend (columns stream front to back)"), ("plane", "free clip plane"))

TAKEN = "taken"
RECORD = {"slice_ring": {}, "column_stream": {}}     # case -> TAKEN or the refusal's text
_CASES, _GATHER = {}, {}


def case_of(seed, case):
    """(scene, feature record, checker frame, checker depth or None) of a case: computed once, read-only"""
    key = (seed, case)
    if key not in _CASES:
        sc, ft = F.feature_scene(seed, case)
        if ft["depth"]:
            ref, rd = sc.render(blend=ft["blend"], depth=True)
            rd.setflags(write=False)
        else:
            ref, rd = sc.render(blend=ft["blend"]), None
        ref.setflags(write=False)
        _CASES[key] = (sc, ft, ref, rd)
    return _CASES[key]


def push(R, sc, ft, upload=True):
    push_scene(R, sc, upload=upload)
    R.set_blend(ft["blend"])
    if sc.subbox:
        R.set_region(*region_extents(sc))
    else:
        R.set_region()


def restore(R):
    R.set_option("kernel", 0)
    R.set_option("cols_counts", 0)
    R.set_blend(0)
    R.set_region()
    R.set_clip(0, None)
    R.set_clip_plane(None)
    R.set_perturb(None, None, None)


@contextlib.contextmanager
def context_for(R0, factory, ft):
    """the shared context with everything restored afterwards, or a shard's own (sharded before its first upload)"""
    if not ft["shard"]:
        try:
            yield R0
        finally:
            restore(R0)
        return
    R = factory()
    try:
        halo = F.halo_for(ft)
        if halo:
            R.set_option("halo", halo)
        R.set_shard(*ft["shard"])
        yield R
    finally:
        R.close()


def gather_frame(R, key, ft, smk_error):
    """(rgba, depth or None) of the gather kernel for the case R holds; rendered once per case and process"""
    if key not in _GATHER:
        got, why = forced(R, 1, smk_error, depth=ft["depth"])
        assert why is None and R.last_frame_info()[0] == 1, why
        _GATHER[key] = got if ft["depth"] else (got, None)
    return _GATHER[key]


def render(R, smk_error, **kw):
    """(frame, None), or (None, the planner's reason) when the forced kernel does not take the frame.  An error of the HIP
    runtime ends the session: nothing more is started on a GPU that has faulted"""
    try:
        return R.render(**kw), None
    except smk_error as e:
        if " failed: " in str(e):
            pytest.exit("HIP runtime error, the session ends here: " + str(e), returncode=3)
        if "not applicable: " not in str(e):
            raise
        return None, str(e).split("not applicable: ", 1)[1]


def forced(R, kernel, smk_error, **kw):
    R.set_option("kernel", kernel)
    return render(R, smk_error, **kw)


def cols_prediction(ft):
    """the mode refusal of cols_refusal (smk_cols_plan.hip), in its order, or None"""
    on = {"pert": ft["pert"], "btf": ft["blend"] == 1, "plane": ft["cut"] == "plane"}
    return next((text for k, text in COLS_MODES if on[k]), None)


def leg_gather(R, key, sc, ft, ref, rd, smk_error, tag):
    push(R, sc, ft)
    ga, gd = gather_frame(R, key, ft, smk_error)
    err = np.abs(ga - ref).max()
    print(tag + ": gather vs checker %g" % err)
    assert err <= TOL, tag + ": gather kernel vs CPU checker %g" % err
    if ft["depth"]:
        _depth_rule(rd, gd)
    return err


def leg_slice_ring(R, key, sc, ft, ref, smk_error, tag):
    """TAKEN or the refusal"""
    push(R, sc, ft)
    ga, gd = gather_frame(R, key, ft, smk_error)
    b, why = forced(R, 2, smk_error)
    assert R.stat("slab_status") == 0, tag
    if ft["pert"]:
        assert why == "perturbation", tag + ": " + str(why)
        return why
    if why is not None:
        assert why in SLAB_GEOMETRIC, tag + ": slice-ring kernel refused for no reason of geometry: " + why
        return why
    assert R.last_frame_info()[0] == 2, tag
    d, e = np.abs(b - ga).max(), np.abs(b - ref).max()
    print(tag + ": slice-ring vs gather %g, vs checker %g" % (d, e))
    if ft["blend"] == 1:
        assert d <= TOL_G, tag + ": slice-ring vs gather %g" % d
    else:
        assert np.array_equal(b, ga), tag + ": slice-ring vs gather %g" % d
    assert e <= TOL, tag + ": slice-ring kernel vs CPU checker %g" % e
    if ft["depth"]:
        (b2, sd), why2 = forced(R, 2, smk_error, depth=True)
        assert why2 is None, tag + ": taken without the depth request, refused with it: " + str(why2)
        assert R.stat("slab_status") == 0, tag
        assert np.array_equal(b2, b), tag + ": the depth request changed the frame by %g" % np.abs(b2 - b).max()
        fin = np.isfinite(gd)
        assert np.array_equal(fin, np.isfinite(sd)), tag + ": depth is finite at other pixels"
        assert np.array_equal(gd[fin], sd[fin]), tag + ": depth differs by %g" % np.abs(gd[fin] - sd[fin]).max()
    return TAKEN


def _cols_frame(R, smk_error):
    R.set_option("cols_counts", 1)
    flagged = R.stat("slab_failures")       # (a context's count of flagged frames: this frame must not add to it)
    b, why = forced(R, 3, smk_error)
    assert R.stat("slab_status") == 0
    if why is None:
        assert R.last_frame_info()[0] == 4
        assert R.stat("slab_failures") == flagged
    return b, why


def leg_column_stream(R, key, sc, ft, ref, smk_error, tag, again=False):
    """TAKEN or the refusal; again: render once more in another window without a new upload"""
    push(R, sc, ft)
    ga, _ = gather_frame(R, key, ft, smk_error)
    b, why = _cols_frame(R, smk_error)
    want = cols_prediction(ft)
    if want is not None:
        assert why == want, tag + ": expected '%s', got %s" % (want, why)
        return why
    if why is not None:
        assert why in COLS_GEOMETRIC, tag + ": column-stream kernel refused for no reason of geometry: " + why
        return why
    d, e = np.abs(b - ga).max(), np.abs(b - ref).max()
    print(tag + ": column-stream vs gather %g, vs checker %g" % (d, e))
    if ft["blend"] == 2:
        assert np.array_equal(b, ga), tag + ": column-stream vs gather %g" % d
    assert d <= TOL_G, tag + ": column-stream vs gather %g" % d
    assert e <= TOL, tag + ": column-stream kernel vs CPU checker %g" % e
    if again:
        w, h = sc.width, sc.height
        try:
            sc.width, sc.height = 3 * w // 2 + 1, max(9, 2 * h // 3 + 2)
            ref2 = sc.render(blend=ft["blend"])
            push(R, sc, ft, upload=False)
            ga2, _ = forced(R, 1, smk_error)
            b2, why2 = _cols_frame(R, smk_error)
            if why2 is not None:
                assert why2 in COLS_GEOMETRIC, tag + ": second window refused for no reason of geometry: " + why2
            else:
                d, e = np.abs(b2 - ga2).max(), np.abs(b2 - ref2).max()
                print(tag + ": second window %dx%d: column-stream vs gather %g, vs checker %g" % (sc.width, sc.height, d, e))
                assert d <= TOL_G and (ft["blend"] != 2 or np.array_equal(b2, ga2)), tag + ": second window vs gather %g" % d
                assert e <= TOL, tag + ": second window vs CPU checker %g" % e
        finally:
            sc.width, sc.height = w, h
    return TAKEN


@pytest.fixture(scope="module")
def R0(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.mark.parametrize("case", range(NCASES))
def test_gather(R0, gpu_renderer_factory, smk, case):
    sc, ft, ref, rd = case_of(SEED, case)
    with context_for(R0, gpu_renderer_factory, ft) as R:
        leg_gather(R, (SEED, case), sc, ft, ref, rd, smk.SmkError, F.describe(ft))


@pytest.mark.parametrize("case", range(NCASES))
def test_slice_ring(R0, gpu_renderer_factory, smk, case):
    sc, ft, ref, _ = case_of(SEED, case)
    with context_for(R0, gpu_renderer_factory, ft) as R:
        RECORD["slice_ring"][case] = "failed"
        RECORD["slice_ring"][case] = leg_slice_ring(R, (SEED, case), sc, ft, ref, smk.SmkError, F.describe(ft))


@pytest.mark.parametrize("case", range(NCASES))
def test_column_stream(R0, gpu_renderer_factory, smk, case):
    sc, ft, ref, _ = case_of(SEED, case)
    with context_for(R0, gpu_renderer_factory, ft) as R:
        RECORD["column_stream"][case] = "failed"
        again = sum(v == TAKEN for v in RECORD["column_stream"].values()) % 4 == 0
        RECORD["column_stream"][case] = leg_column_stream(R, (SEED, case), sc, ft, ref, smk.SmkError, F.describe(ft), again=again)


def tally(leg, eligible):
    """(taken, refused, {reason: count}) of a leg over the eligible cases"""
    got = [RECORD[leg][c] for c in range(NCASES) if eligible(F.draw(SEED, c))]
    reasons = {}
    for v in got:
        if v != TAKEN:
            reasons[v] = reasons.get(v, 0) + 1
    return sum(v == TAKEN for v in got), len(got) - sum(v == TAKEN for v in got), reasons


def test_tally():
    """Conditions, not measurements: of the unperturbed cases the slice-ring kernel took at least half (the bar of
    test_random_frames), of the cases the column-stream kernel takes by mode it took at least half.  A leg is judged when
    every one of its cases ran in this process."""
    legs = [(leg, el) for leg, el in (("slice_ring", lambda ft: not ft["pert"]), ("column_stream", F.cols_by_mode))
            if len(RECORD[leg]) == NCASES]
    if not legs:
        pytest.skip("no leg ran every case in this process")
    for leg, eligible in legs:
        took, refused, reasons = tally(leg, eligible)
        print("%s kernel took %d of its %d frames, refused %d: %s" % (leg, took, took + refused, refused, reasons))
    for leg, eligible in legs:
        took, refused, reasons = tally(leg, eligible)
        assert 2 * took >= took + refused, "%s kernel refused %d of %d frames: %s" % (leg, refused, took + refused, reasons)
