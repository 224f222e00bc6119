"""Half-angle shadows for perturbed fetches (option shadow_perturb) and sub-boxes (smk_set_region): the product's frames,
light buffers, per-slice light history and first-hit depth against the float64 slice pipeline with the displaced fetch and
the sub-box (tests/_shadow_pert_ref.py), under the bounds of tests/test_shadow_witness.py.

Tolerance of a perturbed frame (derived, not measured): the project's TOL bounds placement error x table slope; the displaced
fetch position is Lipschitz in the sample's own position with K = 1 + sum_q w_q s_q n g (_shadow_pert_ref.lipschitz, from the
test's own noise array), so a placement error reaches the table K times larger: K TOL, and 2 K TOL for the mid-frame history
as tests/test_gpu_shadow_witness.py has it.  Sub-box frames without perturbation: K = 1."""
import numpy as np
import pytest

import _present_ref as PR
import _shadow_pert_ref as ref
from _scenes import make_scene, push_scene
from test_shadow_witness import LIGHTS, TOL, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def RM(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.fixture
def R(RM):
    yield RM
    for key, value in (("kernel", 0), ("shadow_march", 1), ("shadow_fused", 0), ("bricks", 1), ("shadow_perturb", 0)):
        RM.set_option(key, value)
    RM.set_region()
    RM.set_perturb(None, None, None)
    RM.set_shadow(0)


def _push(R, sc, option=1):
    push_scene(R, sc)
    if tuple(sc.region[0]) == (0, 0, 0) and tuple(sc.region[1]) == tuple(sc.dims):
        R.set_region()
    else:
        R.set_region(*ref.region_extents(sc))
    R.set_option("shadow_perturb", option)


def _paths(R, kernels=(1, 0), auto_is=(1,), hist=()):
    """name -> (frame, light buffer, {k: history buffer}) for the forced kernels, auto mode (kernel 0) and a launch per slice
    (which keeps no history: its light buffer IS the buffer after the last slice)"""
    out = {}
    try:
        for kern in kernels:
            R.set_option("kernel", kern)
            f, lb = R.render(), R.light_buffer()
            assert R.last_frame_info()[0] in ((kern,) if kern else auto_is), (kern, R.last_frame_info()[0])
            out["kernel %d" % kern] = (f, lb, {k: R.light_history(k) for k in hist})
        R.set_option("kernel", 0)
        R.set_option("shadow_march", 0)
        out["per slice"] = (R.render(), R.light_buffer(), {})
        assert R.last_frame_info()[0] == 3
    finally:
        R.set_option("shadow_march", 1)
        R.set_option("kernel", 0)
    return out


def _hold(R, sc, w, K, kernels=(1, 0), auto_is=(1,)):
    S = w["nslices"]
    ks = ((1, K * TOL), (S // 2, 2 * K * TOL), (S, K * TOL))
    paths = _paths(R, kernels, auto_is, hist=[k for k, _ in ks])
    for name, (got, gotL, hist) in paths.items():
        try:
            compare(got, gotL, w, tol=K * TOL, ltol=K * TOL)
            for k, tol in ks:
                if k in hist:
                    d = np.abs(hist[k] - w["history"][k]).max(axis=2)[~w["lamb_history"][k]]
                    assert d.max(initial=0) <= tol, f"light_history({k}): max {d.max(initial=0)} > {tol}"
        except AssertionError as e:
            raise AssertionError(f"{name}, K = {K:.3f} (tolerance {K * TOL:.3g}): {e}") from None
    return paths


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_perturbed_frames_buffers_and_history_equal_the_witness(R, O, name):
    """kernel 1, auto mode (which must land on kernel 1: the slice-ring kernel declines perturbed frames) and a launch per
    slice; the ragged case has a 35^2 light buffer (no multiple of the march's 8 x 4 texel blocks), `noise24` a noise texture
    that is no power of two (the general wrap-around of smk_noise)"""
    sc, w = ref.witness(name)
    _push(R, sc)
    _hold(R, sc, w, ref.lipschitz(sc))


@pytest.mark.parametrize("name", ["cfg3-u8-shade-oblique-rot", "cfg3-f32-shade-behind-back", "noise24"])
def test_two_marches_equal_a_launch_per_slice_bit_for_bit(R, O, name):
    """the claim of tests/test_gpu_shadow.py::test_two_marches_equal_a_launch_per_slice for perturbed frames: the same
    displaced fetch in the light march, the gather kernel's eye pass and both passes of the per-slice form"""
    sc, w = ref.witness(name)
    _push(R, sc)
    S = w["nslices"]
    p = _paths(R, hist=(1, S // 2, S))
    f, lb, hist = p["kernel 1"]
    fa, lba, hista = p["kernel 0"]
    b, lbb, _ = p["per slice"]
    assert b[..., 3].max() > 0.05 and lbb[..., 3].max() > 0.05, "vacuous scene"
    assert np.array_equal(f, fa) and np.array_equal(lb, lba) and all(np.array_equal(hist[k], hista[k]) for k in hist)
    assert np.array_equal(lb, lbb) and np.array_equal(hist[S], lbb)
    assert bool(R.shadowcoef().front_to_back) == w["front_to_back"]
    if w["front_to_back"]:
        assert np.array_equal(f, b)
    else:
        assert np.abs(f - b).max() <= 2e-5


def _sparse_scene():
    """a table that paints the upper half of the values only: 2 % of the voxels; five in six of the 48^3 volume's 8^3 bricks
    hold nothing visible, one in five has no visible brick next to it either (the dilated flags' case)"""
    sc = make_scene("cfg3", n=48, size=48, steps=60, pose="rot", f32=True, shade=1, pert=True)
    tf = np.zeros((256, 256, 4), np.uint8)
    tf[:, 128:] = (230, 160, 60, 140)
    sc.tf_vg = tf
    sc.light_pos = LIGHTS["oblique"]
    sc.shadow = (64, 0.5)
    return sc


def test_brick_flags_change_nothing(R, O):
    """option bricks 0 against 1: the dilated flags at a sample's own position and the plain ones at the displaced cell skip
    exactly transparent samples only -- frames, light buffers and history identical, in both forms"""
    sc = _sparse_scene()
    _push(R, sc)
    S = int(R.shadowcoef().nslices)
    out = {}
    for bricks in (1, 0):
        R.set_option("bricks", bricks)
        out[bricks] = _paths(R, kernels=(1,), hist=(S // 2, S))
    f, lb, _ = out[1]["kernel 1"]
    assert f[..., 3].max() > 0.05 and lb[..., 3].max() > 0.05, "vacuous scene"
    assert (f[..., 3] > 0).mean() < 0.5                       # (the frame is mostly empty: there are bricks to skip)
    for name in out[1]:
        for a, b in zip(out[1][name][:2], out[0][name][:2]):
            assert np.array_equal(a, b), name
        for k in out[1][name][2]:
            assert np.array_equal(out[1][name][2][k], out[0][name][2][k]), (name, k)
    vox = np.asarray(sc.data[..., 0], np.float32)
    cells = vox[:48, :48, :48].reshape(6, 8, 6, 8, 6, 8).max(axis=(1, 3, 5))
    assert (cells < 0.45).mean() > 0.5                        # most bricks lie below the table's support (from 127 / 256 on)


def test_zero_weights_and_a_whole_volume_region_are_the_plain_frame(R, O):
    sc = ref.case_scene("cfg3-f32-shade-behind-back", pert=False)
    _push(R, sc, option=0)
    want = _paths(R, auto_is=(1, 2))
    sc.noise, sc.pert_w = O.noise_tex(32), (0, 0, 0, 0)       # (c) the option on, every weight 0
    _push(R, sc, option=1)
    got = _paths(R, auto_is=(1, 2))
    for name in want:
        assert np.array_equal(got[name][0], want[name][0]) and np.array_equal(got[name][1], want[name][1]), name
    sc.noise = None
    push_scene(R, sc)
    R.set_region((0, 0, 0), tuple(float(f) for f in sc.fsize))  # (d) a region equal to the whole volume
    got = _paths(R, kernels=(1, 2, 0), auto_is=(1, 2))
    for name in want:
        assert np.array_equal(got[name][0], want[name][0]) and np.array_equal(got[name][1], want[name][1]), name
    assert np.array_equal(got["kernel 2"][1], want["kernel 1"][1])


def test_sub_box_frames_equal_the_witness(R, O):
    """a region cut on two axes, no perturbation (K = 1): the gather kernel, the slice-ring kernel, auto mode and a launch per
    slice; then the same region with a free clip plane"""
    for name in ("region", "region-free-plane"):
        sc, w = ref.witness(name)
        _push(R, sc, option=0)                                # (the sub-box needs no switch)
        paths = _hold(R, sc, w, 1.0, kernels=(1, 2, 0), auto_is=(1, 2))
        assert np.array_equal(paths["kernel 1"][1], paths["per slice"][1])
    plain = ref.case_scene("region")
    plain.region = ((0, 0, 0), tuple(plain.dims))
    _push(R, plain, option=0)
    assert np.abs(R.render() - ref.witness("region")[1]["rgba"]).max() > 0.05     # (the sub-box IS another frame)


def test_sub_box_with_perturbation_equals_the_witness(R, O):
    sc, w = ref.witness("region-pert")
    _push(R, sc)
    _hold(R, sc, w, ref.lipschitz(sc))


def test_sample_counts_follow_the_boxes_not_the_noise(R, O):
    """smk_count_samples and light_samples of a sub-box frame with shadows: fewer than the whole volume's, and the same with
    and without perturbation (only the fetch is displaced)"""
    sc = ref.case_scene("region-pert")
    _push(R, sc)
    n_eye, n_light = R.count_samples(), R.stat("light_samples")
    sc.noise = None
    _push(R, sc)
    assert (R.count_samples(), R.stat("light_samples")) == (n_eye, n_light)
    R.set_region()
    assert R.count_samples() > n_eye > 0 and R.stat("light_samples") > n_light > 0


@pytest.mark.parametrize("name", ["cfg3-u8-shade-oblique-rot", "cfg3-f32-shade-behind-back"])
def test_depth_equals_the_witness(R, O, name):
    """first-hit depth of a perturbed frame with shadows on unambiguous pixels: the view depth of the nearest sample's OWN
    position (the noise moves the fetch, not the fragment)"""
    sc, w = ref.witness(name)
    _push(R, sc)
    _, d = R.render(depth=True)
    ok = ~w["amb"]
    fin = np.isfinite(w["depth"]) & ok
    assert fin.sum() >= 100
    assert np.array_equal(np.isfinite(d[ok]), np.isfinite(w["depth"][ok]))
    assert np.abs(d[fin] - w["depth"][fin]).max() <= 1e-4


def _fresh_plain(gpu_renderer_factory, sc):
    r = gpu_renderer_factory()
    try:
        push_scene(r, sc)
        return r.render(), r.light_buffer()
    finally:
        r.close()


def test_opt_in_and_refusals(R, O, smk, gpu_renderer_factory):
    import torch
    plain = ref.case_scene("cfg3-u8-shade-oblique-rot", pert=False)
    want, wantL = _fresh_plain(gpu_renderer_factory, plain)

    def plain_frame_is_untouched():
        _push(R, plain, option=0)
        assert np.array_equal(R.render(), want) and np.array_equal(R.light_buffer(), wantL)

    sc = ref.case_scene("cfg3-u8-shade-oblique-rot")
    _push(R, sc, option=0)                                    # the default: refused as before
    with pytest.raises(smk.SmkError, match="perturbation"):
        R.render()
    plain_frame_is_untouched()
    _push(R, sc, option=1)
    R.set_option("shadow_fused", 1)                           # the developer option has no perturbed instances
    with pytest.raises(smk.SmkError, match="shadow_fused"):
        R.render()
    R.set_option("shadow_fused", 0)
    plain_frame_is_untouched()
    _push(R, sc, option=1)
    R.set_option("kernel", 2)                                 # forced slice-ring: fails as without shadows
    with pytest.raises(smk.SmkError, match="perturbation"):
        R.render()
    R.set_option("kernel", 0)
    plain_frame_is_untouched()
    # a two-rank shard context: refused, naming shards, in both phases -- perturbation and sub-box alike
    r2 = gpu_renderer_factory()
    try:
        r2.set_shard(0, 2)
        r2.set_option("halo", 12)
        exports = torch.zeros((2, 32, 32, 4), dtype=torch.float32, device="cuda")
        for what in ("pert", "region"):
            s2 = ref.case_scene("cfg3-u8-shade-oblique-rot" if what == "pert" else "region")
            _push(r2, s2, option=1)
            with pytest.raises(smk.SmkError, match="shadows on shards"):
                r2.render()
            with pytest.raises(smk.SmkError, match="shadows on shards"):
                r2.shadow_exports_device(exports.data_ptr())
            torch.cuda.synchronize()
    finally:
        r2.close()
    plain_frame_is_untouched()


def test_occluded_and_present_compose_with_the_new_frames(R, O):
    sc, w = ref.witness("cfg3-u8-shade-oblique-rot")
    _push(R, sc)
    frame, depth = R.render(depth=True)
    hit = np.isfinite(depth)
    assert hit.sum() >= 100
    # a scene depth behind everything: the same frame, bit for bit
    far = np.full(depth.shape, 19.0, np.float32)
    got, gd = R.render(depth=True, scene_depth=far)
    assert np.array_equal(got, frame) and np.array_equal(gd, depth)
    # a depth plane through the volume: every fragment lies in front of it, and nothing in front of it is lost
    zp = float(np.median(depth[hit]))
    plane = np.full(depth.shape, zp, np.float32)
    occ, od = R.render(depth=True, scene_depth=plane)
    seen = np.isfinite(od)
    assert seen.any() and (od[seen] < zp).all() and not seen[~hit].any()
    assert np.array_equal(od[seen], depth[seen])              # (slices run away from the viewer: the first hit is the same)
    assert (occ[..., 3] <= frame[..., 3] + 1e-6).all() and (occ[..., 3] < frame[..., 3] - 1e-3).any()
    assert not occ[hit & (depth >= zp)].any()
    # the display-ready frame is the present rule of the float frame
    rgba8 = R.render_present()
    assert np.array_equal(rgba8, PR.present_rgba8(frame))
