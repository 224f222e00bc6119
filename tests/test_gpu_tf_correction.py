"""The product's default classification path, end to end: with option "tf_raw" 0 every frame derives a correction rate
from its sampling (and, in steps mode, from its view), builds copyScale's alpha map, has smk_k_tf_effective apply it to
the raw (V,G) table on the device and write the occupancy bitmap, rotates the result through four versions behind stream
events, rebuilds that version's brick flags -- and skips all of it when the new map equals the applied one.

Here the product gets the RAW table; the CPU checker gets the table tests/_tf_correction.py corrected in numpy float64 with
the rate smk.h documents, computed from the checker's own ray set-up.  Bounds are the project's: <= 1e-4 against the
checker on premultiplied fp32 RGBA, gather and slice-ring kernels bit-identical, column-stream <= 2e-5 from gather.
No case passes vacuously: the checker's frame has alpha > 0.05 somewhere and moves by more than 1e-2 when the table is
left uncorrected.  In steps mode gamma is picked so that the effective rate is outside [0.8, 1.25].  The sample-rate
grid is fixed and has rates inside: 1.2 and 1.136 still move the checker's frame by 0.056 and more; at a rate of exactly
1 (gamma 1 with sample rate 1 or without scale_alphas) the map is the identity but for 42 bytes that floor() takes one
down, which moves the frame by 0.0086 to 0.053 -- there the floor is ten tolerances, 1e-3, and the map must differ from
the identity: an uncorrected table would still fail the comparison ten times over.

smk_get_tf2d_effective re-applies the map on the host, so its table says nothing about the kernel; what pins the kernel
is the frames (every texel a sample fetches), the brick flags (the bitmap it ballots) and the exactly-zero band pixels."""
import copy

import numpy as np
import pytest

import _tf_correction as T
from _scenes import make_scene, vgh_volume

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_G = 2e-5
KERNEL_ID = {1: 1, 2: 2, 3: 4}      # what last_frame_info reports for option "kernel" 1 / 2 / 3
ERRS = {}                           # the running test's largest error per group


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _measured(record_property):
    """the test's largest errors as properties of its report (--junitxml keeps them, captured output or not)"""
    ERRS.clear()
    yield
    for k in sorted(ERRS):
        record_property("max abs err, " + k, float("%.3g" % ERRS[k]))


def _note(group, err):
    ERRS[group] = max(ERRS.get(group, 0.0), float(err))


def _same_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


def _near_one(rate):
    return 0.8 <= float(rate) <= 1.25


def _reference(sc, raw, moves=1e-2):
    """the checker's frame under the corrected table (sc.tf_vg), with the two assertions against a vacuous case"""
    ref = sc.render()
    assert ref[..., 3].max() > 0.05, "vacuous scene"
    eff, sc.tf_vg = sc.tf_vg, raw
    try:
        plain = sc.render()
    finally:
        sc.tf_vg = eff
    d = np.abs(plain - ref).max()
    assert d > moves, "the correction moves the frame by %g only" % d
    return ref


def _table_matches(r, raw, rate):
    eff, got = r.tf2d_effective(raw.shape[1], raw.shape[0])
    assert _same_bits(got, rate), "rate %r, the checker scene's is %r" % (got, rate)
    assert np.array_equal(eff, T.apply(raw, rate))


def _frames(r, ref, kernels, group):
    """one frame per forced kernel, each against the checker and against one another; returns the gather kernel's"""
    out = {}
    try:
        for k in kernels:
            r.set_option("kernel", k)
            out[k] = r.render()
            assert r.last_frame_info()[0] == KERNEL_ID[k]
            e = np.abs(out[k] - ref).max()
            _note(group + ", checker", e)
            assert e <= TOL, "kernel %d: max abs err %g" % (k, e)
        assert r.stat("slab_failures") == 0
    finally:
        r.set_option("kernel", 0)
    if 2 in out:
        assert np.array_equal(out[1], out[2]), "gather and slice-ring kernels differ by %g" % np.abs(out[1] - out[2]).max()
    if 3 in out:
        e = np.abs(out[3] - out[1]).max()
        _note(group + ", column-stream against gather", e)
        assert e <= TOL_G, "column-stream against gather: %g" % e
    return out[1]


def _want_flags(sc, eff):
    import bricks as B      # oracle/bricks.py
    vol = sc.data
    if vol.dtype == np.uint8:
        v = vol[..., 0].astype(np.float32) * np.float32(1.0 / 255.0)
        g = vol[..., 1].astype(np.float32) * np.float32(1.0 / 255.0)
    else:
        v, g = vol[..., 0].astype(np.float32), vol[..., 1].astype(np.float32)
    return B.brick_flags(np.ascontiguousarray(v), np.ascontiguousarray(g), B.occupancy(eff[..., 3]))


# ------------------------------------------------------------------------------ 1. rates and gamma, sample-rate mode

RATES = (0.6, 1.0, 2.5, 7.3)
GAMMAS = (0.5, 1.0, 2.2)


@pytest.mark.parametrize("kind", ["cfg3", "cfg4"])
@pytest.mark.parametrize("scale_alphas", [1, 0])
@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("sample_rate", RATES)
def test_rates_and_gamma_in_sample_rate_mode(R, sample_rate, gamma, scale_alphas, kind):
    """rate = sample_rate / gamma, or 1 / gamma without scale_alphas -- then the sample rate must not matter: the table is
    the same at another rate, and (in steps mode, where the sample rate does not place the planes either) so is the frame,
    bit for bit.  Voxel type alternates over the grid; the column-stream kernel runs on the gamma 2.2 third."""
    f32 = (RATES.index(sample_rate) + GAMMAS.index(gamma) + (kind == "cfg4")) % 2 == 0
    sc = make_scene(kind, n=32, size=48, pose="rot", f32=f32, shade=1)
    sc.steps, sc.sample_rate = 0, sample_rate
    raw = sc.tf_vg.copy()
    rate = T.push_corrected(R, sc, raw, gamma, scale_alphas)
    want = np.float32(sample_rate) / np.float32(gamma) if scale_alphas else np.float32(1) / np.float32(gamma)
    assert _same_bits(rate, want)
    if float(rate) == 1.0:
        assert (T.alpha_map(rate) != np.arange(256)).sum() >= 32 and not np.array_equal(sc.tf_vg, raw)
    ref = _reference(sc, raw, moves=10 * TOL if float(rate) == 1.0 else 1e-2)
    _table_matches(R, raw, rate)
    _frames(R, ref, (1, 2, 3) if gamma == 2.2 else (1, 2), "sample-rate mode")
    if not scale_alphas:
        other = 0.6 if sample_rate == 2.5 else 2.5
        R.set_sampling(other, 0, gamma, 0)
        _table_matches(R, raw, rate)
        R.set_sampling(sample_rate, 48, gamma, 0)
        a = R.render()
        R.set_sampling(other, 48, gamma, 0)
        b = R.render()
        assert np.array_equal(a, b)
        sc.steps = 48
        assert np.abs(a - sc.render()).max() <= TOL


# ------------------------------------------------------------------------------ 2. steps mode follows the view

def _gamma_for(rate_at_gamma_one):
    """gamma 1 where the view's own rate is well away from 1, else 2.2 (which takes [0.7, 1.4] to [0.32, 0.64])"""
    return 2.2 if 0.7 <= float(rate_at_gamma_one) <= 1.4 else 1.0


def _steps_case(r, sc, kernels, group):
    raw = sc.tf_vg.copy()
    gamma = _gamma_for(T.frame_rate(sc, 1.0, 1))
    rate = T.push_corrected(r, sc, raw, gamma, 1)
    assert not _near_one(rate)
    ref = _reference(sc, raw)
    _table_matches(r, raw, rate)
    _frames(r, ref, kernels, group)
    return rate


@pytest.mark.parametrize("pose", ["id", "rot", "diag", "z-", "x+"])
@pytest.mark.parametrize("steps", [24, 48, 131])
def test_steps_mode_follows_the_view(R, steps, pose):
    f32 = (steps + len(pose)) % 2 == 0
    sc = make_scene("cfg3", n=32, size=56, steps=steps, pose=pose, f32=f32, shade=1)
    _steps_case(R, sc, (1, 2, 3) if steps == 48 else (1, 2), "steps mode")


def test_steps_mode_on_a_volume_with_unequal_axes(R):
    """40 x 24 x 18: fsize / N differs per axis and the view-depth extent swings with the pose (2.67 at `id` against 1.26
    at `rot`, 48 steps)"""
    rates = {}
    for pose, f32 in (("id", True), ("rot", False), ("x+", True)):
        sc = make_scene("cfg3", dims=(40, 24, 18), size=56, steps=48, pose=pose, f32=f32, shade=1)
        rates[pose] = T.frame_rate(sc, 1.0, 1)
        _steps_case(R, sc, (1, 2, 3), "steps mode")
    assert rates["id"] > 2 * rates["rot"]


# ------------------------------------------------------------------------------ 3. alphas the correction removes or creates

def _band_scene(f32, sample_rate):
    """config 3's volume with its first 12 voxel columns set to ONE value, in the middle of ramp_table's alpha 1-2 band:
    rays that stay in there classify inside the band at every sample"""
    sc = make_scene("cfg3", n=32, size=48, pose="id", f32=f32, shade=1)
    sc.steps, sc.sample_rate = 0, sample_rate
    data = sc.data.copy()
    data[:, :, :12, 0] = np.float32(80.0 / 255.0) if f32 else 80
    sc.data = data
    return sc


def _band_pixels(sc):
    """pixels whose every sample classifies inside the band, found with the checker and two probe tables: opaque outside the
    band -> alpha exactly 0 there, opaque inside -> alpha > 0"""
    lo = T.low_band(256)
    alpha = []
    for inside in (0, 1):
        probe = np.full((256, 256, 4), 255, np.uint8)
        probe[..., 3] = 255 * inside
        probe[:, lo[0]:lo[1], 3] = 255 * (1 - inside)
        sc.tf_vg = probe
        alpha.append(sc.render()[..., 3])
    return (alpha[1] == 0) & (alpha[0] > 0)


@pytest.mark.parametrize("f32", [False, True])
def test_alphas_the_correction_removes_or_creates(R, f32):
    """at rate 7.3 bytes 1-7 become 0: the band's pixels are exactly 0 and its bricks lose their flags; at 0.6 byte 1 stays 1
    and 2 becomes 3: the pixels are visible and the bricks flagged.  Flags byte for byte against oracle/bricks.py under the
    numpy-corrected table; frames with and without the flags bit-equal on both ray-marchers."""
    raw = T.ramp_table(256, 256)
    flags = {}
    try:
        for sample_rate in (7.3, 0.6):
            sc = _band_scene(f32, sample_rate)
            band = _band_pixels(sc)
            assert band.sum() >= 40, "only %d band pixels" % band.sum()
            R.set_option("bricks", 1)
            rate = T.push_corrected(R, sc, raw, 1.0, 1)
            ref = _reference(sc, raw)
            _table_matches(R, raw, rate)
            got, _ = R.brick_flags()
            want = _want_flags(sc, T.apply(raw, rate))
            assert got.shape == want.shape
            assert np.array_equal(got, want), "%d of %d flags differ" % ((got != want).sum(), got.size)
            flags[sample_rate] = got
            g1 = _frames(R, ref, (1, 2), "band table")
            R.set_option("bricks", 0)
            g0 = _frames(R, ref, (1, 2), "band table")
            assert np.array_equal(g0, g1), "the flags changed the frame"
            if sample_rate > 1:
                assert (ref[band] == 0).all() and (g1[band] == 0).all()
            else:
                assert (ref[band][:, 3] > 0).all() and (g1[band][:, 3] > 0).all()
        assert not np.array_equal(flags[7.3], flags[0.6])
        assert flags[7.3].sum() < flags[0.6].sum()
    finally:
        R.set_option("bricks", 1)


# ------------------------------------------------------------------------------ 4. table sizes at the kernel's edges

@pytest.mark.parametrize("sv,sg", [(256, 256), (64, 64), (100, 37), (33, 2), (2, 1)])
def test_table_sizes(R, smk, sv, sg):
    """smk_k_tf_effective handles 64 texels of a row per wave and ballots two bitmap words, only the first when sv <= 32;
    100 is no multiple of 64 (nor of 32), 37 x ceil(100 / 64) waves is no multiple of the four waves of a block.  The
    slice-ring and column-stream kernels decline a table with fewer than two rows or columns, each saying so; the gather
    kernel takes the one-row table, forced or chosen."""
    declined = {2: "smk_render: slab kernel forced but not applicable: transfer function smaller than 2x2",
                3: "smk_render: column-stream kernel forced but not applicable: transfer function smaller than 2x2"} if sg < 2 else {}
    sc = make_scene("cfg3", n=32, size=48, pose="rot", f32=sv != 64, shade=1)
    sc.steps, sc.sample_rate = 0, 2.5
    raw = T.ramp_table(sv, sg)
    R.set_option("bricks", 1)
    rate = T.push_corrected(R, sc, raw, 1.0, 1)
    ref = _reference(sc, raw)
    _table_matches(R, raw, rate)
    got, _ = R.brick_flags()
    want = _want_flags(sc, T.apply(raw, rate))
    assert np.array_equal(got, want), "%d of %d flags differ" % ((got != want).sum(), got.size)
    frames = {}
    try:
        for k in (1, 2, 3):
            R.set_option("kernel", k)
            if k in declined:
                with pytest.raises(smk.SmkError) as why:
                    R.render()
                assert str(why.value) == declined[k]
                continue
            frames[k] = R.render()      # (a forced kernel that declined any other size would raise here)
            assert R.last_frame_info()[0] == KERNEL_ID[k]
            e = np.abs(frames[k] - ref).max()
            _note("table sizes, checker", e)
            assert e <= TOL, "kernel %d: %g" % (k, e)
    finally:
        R.set_option("kernel", 0)
    if not declined:
        assert np.array_equal(frames[1], frames[2])
        e = np.abs(frames[3] - frames[1]).max()
        _note("table sizes, column-stream against gather", e)
        assert e <= TOL_G, "column-stream against gather: %g" % e
    auto = R.render()
    assert np.abs(auto - ref).max() <= TOL
    if declined:
        assert R.last_frame_info()[0] == KERNEL_ID[1]
    assert R.stat("slab_failures") == 0


# ------------------------------------------------------------------------------ 5. a turning camera, frames enqueued without waiting

class _Spec:
    def __init__(self, angle, table, step, tf_raw, event):
        self.angle, self.table, self.step, self.tf_raw, self.event = angle, table, step, tf_raw, event


def _turning_sequence(big, small, rate_at):
    """30 frames about pose `rot` (30 degrees about (1, 1, 0)): steps of 3 degrees up and down between 30 and 42 (every one
    changes the map), every third a step of a few thousandths of a degree picked with rate_at(angle) so that it brings a
    new rate and the same map where one does (the test counts the pairs of either kind itself); and the events"""
    specs, wave, fine, up = [], 0, 0.0, 1
    for i in range(30):
        if i and i % 3 == 0:
            before = rate_at(specs[-1].angle)
            for d in (0.004, 0.006, 0.008, 0.003, 0.01, 0.002, 0.012, 0.005, 0.007, 0.009):
                after = rate_at(30.0 + 3.0 * wave + fine + d)
                if after != before and np.array_equal(T.alpha_map(after), T.alpha_map(before)):
                    break
            else:
                d = 0.009       # none at this angle (an alpha byte's threshold is too near): an ordinary pair, with a new map
            fine += d
        elif i:
            if wave + up > 4 or wave + up < 0:
                up = -up
            wave += up
        table = small if i in (0, 1, 12) else big
        event = {2: "table grows", 12: "table shrinks", 13: "table grows back", 19: "time step 1", 21: "time step 0",
                 25: "tf_raw on", 26: "tf_raw off"}.get(i)
        specs.append(_Spec(30.0 + 3.0 * wave + fine, table, 1 if i in (19, 20) else 0, 1 if i == 25 else 0, event))
    return specs


def test_a_turning_camera_without_waiting(gpu_renderer_factory, O):
    """steps mode, slice-ring kernel, brick flags on, frames enqueued into kept buffers with nothing but set_camera between
    them (tf_dirty stays false: the rate comparison and the byte-equal-map test decide what is refreshed).  The sequence
    has pairs with a new rate and the same map (the skip path) and pairs with a new map (a new version: they wrap more than
    twice), and a stale version would show: the checker's frames under the previous and the current table differ by more
    than ten tolerances.  Interleaved: a table that grows and shrinks (the version's capacity), a time-step switch, and
    tf_raw toggled without the table being sent again."""
    import torch
    size, steps, gamma = 48, 48, 2.2
    base = make_scene("cfg3", n=32, size=size, steps=steps, pose="rot", f32=True, shade=1)
    big, small = base.tf_vg.copy(), T.ramp_table(100, 37)
    _, vol1, nrm1 = vgh_volume(32, 2)
    vols = {0: (base.data, base.grad), 1: (vol1, nrm1)}

    def turned(angle):
        sc = copy.copy(base)
        sc.mv_override = O.modelview(base.eye, base.at, base.up, base.trans, O.rotation((1, 1, 0), angle), base.fsize)
        return sc

    specs = _turning_sequence(big, small, lambda angle: T.frame_rate(turned(angle), gamma, 1))
    assert len(specs) >= 24

    def scene(f, rate_of=None):
        sc = turned(f.angle)
        sc.data, sc.grad = vols[f.step]
        rate = T.frame_rate(sc, gamma, 1)
        sc.tf_vg = f.table if f.tf_raw else T.apply(f.table, rate if rate_of is None else rate_of)
        return sc, rate

    scenes, rates = zip(*[scene(f) for f in specs])
    maps = [T.alpha_map(x) for x in rates]
    plain = [i for i in range(1, len(specs)) if specs[i].event is None and specs[i - 1].event != "tf_raw on"]
    skipped = [i for i in plain if rates[i] != rates[i - 1] and np.array_equal(maps[i], maps[i - 1])]
    changed = [i for i in plain if not np.array_equal(maps[i], maps[i - 1])]
    assert len(skipped) >= 4, "pairs that take the skip path: %s" % skipped
    assert len(changed) >= 8, "pairs with a new map: %s" % changed
    refs = [sc.render() for sc in scenes]
    for i in changed:
        stale, _ = scene(specs[i], rate_of=rates[i - 1])
        d = np.abs(stale.render() - refs[i]).max()
        assert d > 10 * TOL, "frame %d: a stale table would move it by %g only" % (i, d)
    for i, f in enumerate(specs):
        assert refs[i][..., 3].max() > 0.05
        if not f.tf_raw:
            un = copy.copy(scenes[i])
            un.tf_vg = f.table
            assert np.abs(un.render() - refs[i]).max() > 1e-2

    def camera(r, sc):
        r.set_camera(sc.mv(), sc.frustum, (sc.znear, 20.0), sc.width, sc.height)

    r = gpu_renderer_factory()
    try:
        r.set_timestep_cache(2)
        first = copy.copy(scenes[0])
        T.push_corrected(r, first, specs[0].table, gamma, 1)
        r.upload_timestep(1, vol1, nrm1, fsize=tuple(float(v) for v in base.fsize), dmode="VGH")
        r.set_option("bricks", 1)
        r.set_option("kernel", 2)
        bufs = [torch.zeros((size * size, 4), dtype=torch.float32, device="cuda") for _ in specs]
        for i, f in enumerate(specs):
            if i:
                p = specs[i - 1]
                if f.table is not p.table:
                    r.set_tf2d(f.table, None)
                if f.step != p.step:
                    r.select_timestep(f.step)
                if f.tf_raw != p.tf_raw:
                    r.set_option("tf_raw", f.tf_raw)
            camera(r, scenes[i])
            r.render_device(bufs[i].data_ptr())
        torch.cuda.synchronize()
        assert r.stat("slab_failures") == 0
        got = [b.cpu().numpy().reshape(size, size, 4) for b in bufs]
        for i, f in enumerate(specs):
            e = np.abs(got[i] - refs[i]).max()
            _note("turning camera, checker", e)
            assert e <= TOL, "frame %d (%s): max abs err %g" % (i, f.event, e)
        r.set_option("kernel", 1)
        r.set_option("bricks", 0)
        for i, f in enumerate(specs):
            r.set_tf2d(f.table, None)
            r.select_timestep(f.step)
            r.set_option("tf_raw", f.tf_raw)
            camera(r, scenes[i])
            g = r.render()
            assert r.last_frame_info()[0] == 1
            assert np.array_equal(got[i], g), "frame %d (%s) differs from the gather kernel's by %g" % (i, f.event, np.abs(got[i] - g).max())
            if not f.tf_raw:
                _table_matches(r, f.table, rates[i])
    finally:
        r.close()


# ------------------------------------------------------------------------------ 6. shadows and shards

def test_shadow_frame_in_steps_mode_with_gamma(R):
    """half-angle slicing: the eye pass and the light march classify through the same corrected table"""
    sc = make_scene("cfg3", n=32, size=48, steps=48, pose="rot", f32=True, shade=1)
    sc.light_pos = (3, 4, -3)
    sc.shadow = (128, 0.5)
    raw = sc.tf_vg.copy()
    try:
        rate = T.push_corrected(R, sc, raw, 2.2, 1)
        assert not _near_one(rate)
        ref, ref_l = sc.render_shadow()
        eff, sc.tf_vg = sc.tf_vg, raw
        plain, plain_l = sc.render_shadow()
        sc.tf_vg = eff
        assert ref[..., 3].max() > 0.05 and ref_l[..., 3].max() > 0.05
        assert np.abs(plain - ref).max() > 1e-2 and np.abs(plain_l - ref_l).max() > 1e-2
        _table_matches(R, raw, rate)
        got = R.render()
        got_l = R.light_buffer()
        assert R.last_frame_info()[0] in (1, 2)
        assert got_l.shape == ref_l.shape
        e, e_l = np.abs(got - ref).max(), np.abs(got_l - ref_l).max()
        _note("shadow frame, checker", e)
        _note("shadow light buffer, checker", e_l)
        assert e <= TOL, "frame max abs err %g" % e
        assert e_l <= TOL, "light buffer max abs err %g" % e_l
    finally:
        R.set_shadow(0)


@pytest.mark.parametrize("world", [2, 8])
def test_shards_correct_with_the_unsharded_rate(gpu_renderer_factory, R, world):
    """the rate comes from the WHOLE volume's view-depth extent, whatever part a rank stores"""
    import torch
    sc = make_scene("cfg3", n=32, size=48, steps=48, pose="rot", f32=True, shade=1)
    raw = sc.tf_vg.copy()
    gamma = _gamma_for(T.frame_rate(sc, 1.0, 1))
    rate = T.push_corrected(R, sc, raw, gamma, 1)
    assert not _near_one(rate)
    ref = _reference(sc, raw)
    _table_matches(R, raw, rate)
    whole = R.render()
    npix = sc.width * sc.height
    layers = torch.zeros((world, npix, 4), dtype=torch.float32, device="cuda")
    rs = []
    try:
        for k in range(world):
            r = gpu_renderer_factory()
            rs.append(r)
            r.set_shard(k, world)
            T.push_corrected(r, sc, raw, gamma, 1)
            _table_matches(r, raw, rate)
            r.render_device(layers[k].data_ptr(), None, None)
        torch.cuda.synchronize()
        for r in rs:
            assert r.stat("slab_status") == 0
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        rs[0].composite_over_device(layers.data_ptr(), world, rs[0].shard_order(world), npix, out.data_ptr(), None)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(sc.height, sc.width, 4)
        e, e_w = np.abs(got - ref).max(), np.abs(got - whole).max()
        _note("shards, checker", e)
        _note("shards, unsharded frame", e_w)
        assert e_w <= TOL_G, "merged against unsharded: %g" % e_w
        assert e <= TOL, "merged against the checker: %g" % e
    finally:
        for r in rs:
            r.close()


# ------------------------------------------------------------------------------ 7. refusals

def test_refused_sampling_leaves_the_state_alone(R, smk):
    sc = make_scene("cfg3", n=32, size=48, steps=48, pose="rot", f32=True, shade=1)
    raw = sc.tf_vg.copy()
    rate = T.push_corrected(R, sc, raw, 2.2, 1)
    ref = _reference(sc, raw)
    before = R.render()
    assert np.abs(before - ref).max() <= TOL
    gamma_msg = "smk_set_sampling: gamma must be > 0"
    rate_msg = "smk_set_sampling: need sample_rate > 0 or steps > 0"
    for args, msg in (((0.0, 48, 0.0, 1), gamma_msg), ((2.5, 0, -1.0, 1), gamma_msg), ((0.0, 0, 1.0, 1), rate_msg),
                      ((-2.5, 0, 1.0, 1), rate_msg), ((0.0, -3, 1.0, 0), rate_msg)):
        with pytest.raises(smk.SmkError) as e:
            R.set_sampling(*args)
        assert str(e.value) == msg
        _table_matches(R, raw, rate)
        assert np.array_equal(R.render(), before)
