"""The feature fuzz's generator (tests/_fuzz_features.py) held to what makes it worth rendering, with the CPU checker alone:
at the default seed and case count every value of every feature occurs, the products the hand-picked tests do not reach
occur, the frames show something, a requested depth finds a hit, a cut cuts, and enough cases are left for the column-stream
kernel (which takes no perturbation, no back-to-front blend and no free clip plane).  The thresholds are the conditions;
the generator's shares and sizes are what gets tuned to them."""
import numpy as np
import pytest

import _fuzz_features as F

SEED, N = F.DEFAULT_SEED, F.DEFAULT_NCASES


@pytest.fixture(scope="module")
def feats():
    return [F.draw(SEED, case) for case in range(N)]


@pytest.fixture(scope="module")
def frames(feats, O):
    """per case: (checker frame, depth or None, the frame without the cut or None), rendered once"""
    out = []
    for ft in feats:
        sc = F.build(ft)
        if ft["depth"]:
            img, dep = sc.render(blend=ft["blend"], depth=True)
        else:
            img, dep = sc.render(blend=ft["blend"]), None
        whole = F.build(ft, cut=False).render(blend=ft["blend"]) if ft["cut"] != "none" else None
        out.append((img, dep, whole))
    return out


def test_a_case_is_reproducible_alone(feats):
    assert F.draw(SEED, 17) == feats[17] and F.draw(SEED, 17) != F.draw(SEED + 1, 17)


def test_sizes_stay_small(feats):
    for ft in feats:
        assert all(2 <= d <= 72 for d in ft["dims"])
        assert 9 <= ft["width"] <= 150 and 9 <= ft["height"] <= 150 and ft["width"] != ft["height"]
        assert (6 <= ft["steps"] <= 160 and ft["rate"] == 0) or (ft["steps"] == 0 and ft["rate"] > 0)
        assert ft["kind"] != "cfg1" or (not ft["f32"] and ft["shade"] == 0)
        assert sum(ft[k] is not None for k in ("clip", "plane", "region", "shard")) == (ft["cut"] != "none")
        if ft["region"]:
            g0, g1 = ft["region"]
            assert all(0 <= a and a + 2 <= b <= n for a, b, n in zip(g0, g1, ft["dims"])) and (g0, g1) != ((0, 0, 0), ft["dims"])


@pytest.mark.parametrize("feature,values", [
    ("kind", F.KINDS), ("f32", (False, True)), ("shade", (0, 1, 2)), ("use_spec", (0, 1)), ("blend", (0, 1, 2)),
    ("depth", (False, True)), ("cut", F.CUTS), ("pert", (False, True)), ("thin", (False, True)), ("view", F.VIEWS),
    ("rate_mode", (False, True)), ("big", (False, True))])
def test_every_value_of_every_feature_occurs(feats, feature, values):
    get = {"rate_mode": lambda ft: ft["steps"] == 0, "big": lambda ft: max(ft["dims"]) > 40}.get(feature, lambda ft: ft[feature])
    for v in values:
        n = sum(get(ft) == v for ft in feats)
        assert n >= 3, "%s = %s occurs %d times in %d cases" % (feature, v, n, N)


def test_the_products_occur(feats):
    def some(pred):
        return any(pred(ft) for ft in feats)
    for b in (0, 1, 2):
        assert some(lambda ft: ft["blend"] == b and ft["cut"] == "plane"), "blend %d with a free plane" % b
        assert some(lambda ft: ft["blend"] == b and ft["depth"]), "depth with blend %d" % b
        assert some(lambda ft: ft["blend"] == b and ft["kind"] == "cfg1"), "1-D table with blend %d" % b
    assert some(lambda ft: ft["cut"] == "shard" and ft["thin"]), "a shard with a thin axis"
    for f32 in (False, True):
        assert some(lambda ft: ft["kind"] in ("tf3d", "tf3d_panes") and ft["f32"] == f32), "3-D table with f32 = %s" % f32


def test_frames_show_something(feats, frames):
    n = sum(img[..., 3].max() > 0.05 for img, _, _ in frames)
    assert n >= 0.8 * N, "%d of %d frames reach alpha 0.05" % (n, N)


def test_requested_depth_finds_a_hit(feats, frames):
    got = [np.isfinite(dep).any() for (_, dep, _), ft in zip(frames, feats) if ft["depth"]]
    assert sum(got) >= 0.8 * len(got), "%d of %d depth frames have a finite depth" % (sum(got), len(got))


def test_a_cut_cuts(feats, frames):
    got = [not np.array_equal(img, whole) for (img, _, whole), ft in zip(frames, feats) if ft["cut"] != "none"]
    assert sum(got) >= 0.8 * len(got), "%d of %d cut frames differ from the uncut frame" % (sum(got), len(got))


def test_the_column_stream_kernel_is_fed(feats):
    n = sum(F.cols_by_mode(ft) for ft in feats)
    assert n >= 0.4 * N, "%d of %d cases are column-stream eligible by mode" % (n, N)
