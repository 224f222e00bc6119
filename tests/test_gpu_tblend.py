"""Fractional time (smk.h smk_blend_timesteps): a step blended on the device from two resident steps must be, bit for bit,
the step a FRESH context gets when it uploads the NumPy restatement of the contract (tests/_tblend_ref.py, qualified by
tests/test_tblend_ref_cpu.py) with smk_upload_volume -- under every ray-marcher, with and without brick flags, for every
voxel layout, on shards, with shadows and the perturbed fetch, and when the blend runs on another stream beside frames in
flight.  Steps are the seeds 1 (a), 2 (b) and 3 of 32^3 volumes, 64^2 pixels x 64 planes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _tblend_ref as T
from _step_gpu import RAN, fresh_frame, merged_frame as _merged
from _trex_series import write_series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMODE = {1: "V1", 2: "V1G", 3: "VGH", 4: "V2GH"}
GATHER = (("kernel", 1),)


def upload(R, t, sc, grid=(1, 1, 1)):
    R.upload_timestep(t, sc.data, sc.grad, fsize=tuple(float(f) for f in sc.fsize), grid=grid, dmode=DMODE[sc.nelts])


def ring(factory, sa, sb, cap=4, opts=(), grid=(1, 1, 1)):
    """a context with step 0 = scene sa (current) and step 1 = scene sb resident"""
    from _scenes import push_scene
    R = factory()
    try:
        R.set_timestep_cache(cap)
        push_scene(R, sa, grid=grid)
        for k, v in opts:
            R.set_option(k, v)
        upload(R, 1, sb, grid)
    except Exception:
        R.close()
        raise
    return R


def same(got, want, what=""):
    assert np.array_equal(got, want), "%s: max diff %g" % (what, np.abs(got - want).max())


def ends(dtype, **kw):
    return T.scene(*T.step(dtype, 1, **kw)), T.scene(*T.step(dtype, 2, **kw))


def mid(dtype, w, **kw):
    return T.scene(*T.blended(dtype, 1, 2, w, **kw))


# ---- 1. types x kernels

CASES = [(d, k, b) for d in ("u8", "f32", "u16") for k in (0, 1, 2, 3) for b in (0, 1) if not (d == "u16" and k == 3)]


@pytest.mark.parametrize("dtype, kernel, bricks", CASES)
def test_blend_equals_fresh_upload_of_the_restatement(gpu_renderer_factory, dtype, kernel, bricks):
    opts = (("kernel", kernel), ("bricks", bricks))
    R = ring(gpu_renderer_factory, *ends(dtype), opts=opts)
    try:
        for i, w in enumerate(T.WS_F32 if dtype == "f32" else T.WS_INT):
            want = fresh_frame(gpu_renderer_factory, mid(dtype, w), opts)
            assert want[..., 3].max() > 0.05
            shown = R.timesteps()[0]
            R.blend_timesteps(0, 1, w, 10 + (i & 1))
            assert R.timesteps()[0] == shown        # (a blend does not become current)
            R.select_timestep(10 + (i & 1))
            got = R.render()
            same(got, want, "w %g" % w)
            if kernel:
                assert R.last_frame_info()[0] == RAN[kernel]
            if kernel == 1 and bricks == 1 and i == 0:  # ... and against the CPU checker on the restated volume
                sc = T.scene(*T.blended(dtype, 1, 2, w), checker=True)
                assert np.abs(got - sc.render()).max() <= 1e-4
        assert R.stat("slab_failures") == 0
    finally:
        R.close()


# ---- 2. endpoints

@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
def test_endpoints_reproduce_the_steps(gpu_renderer_factory, dtype):
    sa, sb = ends(dtype)
    fa, fb = (fresh_frame(gpu_renderer_factory, s, GATHER) for s in (sa, sb))
    assert not np.array_equal(fa, fb)
    R = ring(gpu_renderer_factory, sa, sb, opts=GATHER)
    try:
        for w, out, want in ((0.0, 10, fa), (1.0, 11, fb)):
            R.blend_timesteps(0, 1, w, out)
            R.select_timestep(out)
            same(R.render(), want, "w %g" % w)
        if dtype != "f32":                          # a == b: every integer field comes back as it was (a float within an
            R.blend_timesteps(1, 1, 0.3, 10)        # ulp: u + w need not be 1; test_ring_and_refusals has that case)
            R.select_timestep(10)
            same(R.render(), fb, "copy of b")
    finally:
        R.close()


# ---- 3. brick flags

@pytest.mark.parametrize("kind", ["cfg3", "tf3d_panes"])
def test_brick_flags_of_a_blended_step(gpu_renderer_factory, kind):
    sa, sb = (T.scene(*T.step("f32", s), kind=kind) for s in (1, 2))
    sm = T.scene(*T.blended("f32", 1, 2, 0.3), kind=kind)
    flags = [fresh_frame(gpu_renderer_factory, s, render=lambda R: R.brick_flags()[0]) for s in (sa, sm)]
    assert not np.array_equal(flags[0], flags[1])
    R = ring(gpu_renderer_factory, sa, sb)
    try:
        R.render()
        R.blend_timesteps(0, 1, 0.3, 10)
        R.select_timestep(10)
        assert np.array_equal(R.brick_flags()[0], flags[1])
        R.render()
        R.select_timestep(0)
        assert np.array_equal(R.brick_flags()[0], flags[0])
    finally:
        R.close()


# ---- 4. layouts (gather kernel)

ODD = (31, 29, 27)
LAYOUTS = {
    "u8-1ch": dict(dtype="u8", nelts=1), "u8-2ch": dict(dtype="u8", nelts=2), "u8-4ch": dict(dtype="u8", nelts=4),
    "f32-4ch-separate-normals": dict(dtype="f32", nelts=4),
    "f32-4ch-separate-normals-odd": dict(dtype="f32", nelts=4, dims=ODD),     # (a voxel count that is no multiple of 4)
    "u8-no-normals": dict(dtype="u8", normals=False), "f32-no-normals": dict(dtype="f32", normals=False),
    "f32-4ch-no-normals": dict(dtype="f32", nelts=4, normals=False),
    "u8-odd": dict(dtype="u8", dims=ODD), "u16-odd": dict(dtype="u16", dims=ODD),   # (the pad column)
    "u8-odd-bricked": dict(dtype="u8", dims=ODD, grid=(2, 1, 2)), "u16-odd-bricked": dict(dtype="u16", dims=ODD, grid=(2, 1, 2)),
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_layouts(gpu_renderer_factory, name):
    from _scenes import push_scene
    kw = dict(LAYOUTS[name])
    dtype, grid = kw.pop("dtype"), kw.pop("grid", (1, 1, 1))
    sa, sb = ends(dtype, **kw)
    fresh = gpu_renderer_factory()
    try:
        push_scene(fresh, mid(dtype, 0.3, **kw), grid=grid)
        fresh.set_option("kernel", 1)
        want = fresh.render()
    finally:
        fresh.close()
    assert want[..., 3].max() > 0.05
    assert not np.array_equal(want, fresh_frame(gpu_renderer_factory, sa, GATHER))
    R = ring(gpu_renderer_factory, sa, sb, opts=GATHER, grid=grid)
    try:
        R.blend_timesteps(0, 1, 0.3, 10)
        R.select_timestep(10)
        same(R.render(), want, name)
    finally:
        R.close()


# ---- 5. ring and refusals

def test_ring_and_refusals(gpu_renderer_factory, smk):
    sa, sb = ends("f32")
    sc = T.scene(*T.step("f32", 3))
    f3, f7 = (fresh_frame(gpu_renderer_factory, mid("f32", w), GATHER) for w in (0.3, 0.7))
    # a == b is a copy by the contract's arithmetic, (u * x) + (w * x): three roundings of 2^-24 and u + w = 1 +- 2^-25, so a
    # float comes back within 2.5 * 2^-24 of itself, relatively
    bb = T.blended("f32", 2, 2, 0.3)
    assert np.allclose(bb[0], T.step("f32", 2)[0], rtol=2.0 ** -22, atol=0) and np.array_equal(bb[1], T.step("f32", 2)[1])
    fb = fresh_frame(gpu_renderer_factory, T.scene(*bb), GATHER)
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match="no volume"):
            R.blend_timesteps(0, 1, 0.3, 5)
    finally:
        R.close()
    R = ring(gpu_renderer_factory, sa, sb, cap=2, opts=GATHER)
    try:
        for args, why in (((0, 1, 0.3, 0), "in-place"), ((0, 1, 0.3, 1), "in-place"),
                          ((99, 1, 0.3, 5), r"99 \(a\) is not cached"), ((0, 99, 0.3, 5), r"99 \(b\) is not cached"),
                          ((0, 1, -0.1, 5), r"not in \[0, 1\]"), ((0, 1, 1.5, 5), r"not in \[0, 1\]"),
                          ((0, 1, float("nan"), 5), r"not in \[0, 1\]"), ((0, 1, 0.3, -1), ">= 0"),
                          ((0, 1, 0.3, 5), "holds 2 steps.*here 3")):
            with pytest.raises(smk.SmkError, match=why):
                R.blend_timesteps(*args)
        assert R.timesteps() == (0, [0, 1]) and R.stat("tblend_count") == 0
        R.set_timestep_cache(3)
        upload(R, 2, sc)
        R.select_timestep(2)                        # a current step that is neither a nor b is a fourth slot
        with pytest.raises(smk.SmkError, match="holds 3 steps.*here 4"):
            R.blend_timesteps(0, 1, 0.3, 5)
        assert R.timesteps() == (2, [0, 1, 2])
        # a == b: a copy, into the slot a fourth step of capacity leaves empty
        R.set_timestep_cache(4)
        R.blend_timesteps(1, 1, 0.3, 7)
        assert R.timesteps() == (2, [0, 1, 2, 7])
        R.select_timestep(7)
        same(R.render(), fb, "copy of b")
        R.select_timestep(2)
        # ten blends into alternating outputs: a, b and the current step hold three of the four slots, the fourth is the
        # outputs' in turn
        for i in range(10):
            R.blend_timesteps(0, 1, (0.3, 0.7)[i & 1], 5 + (i & 1))
            cur, ids = R.timesteps()
            assert cur == 2 and ids == [0, 1, 2, 5 + (i & 1)], (i, cur, ids)
        assert R.stat("tblend_count") == 11
        R.select_timestep(6)
        same(R.render(), f7, "the tenth blend")
        # a cached output that is not current is overwritten in place, and is then the newest
        R.select_timestep(0)
        upload(R, 2, sc)
        assert R.timesteps() == (0, [0, 1, 6, 2])
        R.blend_timesteps(0, 1, 0.3, 6)
        assert R.timesteps() == (0, [0, 1, 2, 6])
        R.select_timestep(6)
        same(R.render(), f3, "in place")
        # ... and the current one: the next frame shows the blend
        R.blend_timesteps(0, 1, 0.7, 6)
        assert R.timesteps() == (6, [0, 1, 2, 6])
        same(R.render(), f7, "current step overwritten")
    finally:
        R.close()


# ---- 6. asynchronous use

def _device(sc):
    import torch
    return torch.from_numpy(np.array(sc.data)).cuda(), torch.from_numpy(np.array(sc.grad)).cuda()


def test_blend_on_a_second_stream_beside_frames_in_flight(gpu_renderer_factory):
    import torch
    sa, sb = ends("f32")
    want = {0: fresh_frame(gpu_renderer_factory, sa), 10: fresh_frame(gpu_renderer_factory, mid("f32", 0.3)),
            11: fresh_frame(gpu_renderer_factory, mid("f32", 0.7))}
    rend, bl = torch.cuda.Stream(), torch.cuda.Stream()
    R = ring(gpu_renderer_factory, sa, sb)
    try:
        torch.cuda.synchronize()                    # nothing is in flight when the streams start
        outs = []

        def frames(n, t):
            for _ in range(n):
                o = torch.empty((sa.height, sa.width, 4), dtype=torch.float32, device="cuda")
                outs.append((o, t))
                R.render_device(o.data_ptr(), None, ctypes.c_void_p(rend.cuda_stream))
        frames(16, 0)                               # frames of step 0 in flight ...
        R.blend_timesteps(0, 1, 0.3, 10, stream=ctypes.c_void_p(bl.cuda_stream))   # ... while the blend runs beside them
        R.select_timestep(10)
        frames(4, 10)
        R.blend_timesteps(0, 1, 0.7, 11, stream=ctypes.c_void_p(bl.cuda_stream))
        frames(4, 10)
        R.select_timestep(11)
        frames(4, 11)
        R.blend_timesteps(0, 1, 0.3, 11, stream=ctypes.c_void_p(bl.cuda_stream))   # the slot those four read: it waits for them
        frames(2, 11)
        R.select_timestep(0)
        frames(1, 0)
        torch.cuda.synchronize()                    # both streams: read-back
        for i, (o, t) in enumerate(outs):
            same(o.cpu().numpy(), want[10 if (t == 11 and i >= 28) else t], "frame %d (step %d)" % (i, t))
        assert R.stat("slab_failures") == 0
    finally:
        R.close()


def test_a_source_overwritten_right_after_the_blend_was_enqueued(gpu_renderer_factory):
    """the upload into slot a, on a third stream, is ordered behind the blend's reads: the blend is of the OLD step 0"""
    import torch
    sa, sb = ends("f32")
    sc = T.scene(*T.step("f32", 3))
    want_mid, want_c = fresh_frame(gpu_renderer_factory, mid("f32", 0.3)), fresh_frame(gpu_renderer_factory, sc)
    dev = _device(sc)
    rend, bl, up = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    R = ring(gpu_renderer_factory, sa, sb)
    try:
        torch.cuda.synchronize()                    # nothing is in flight when the streams start
        outs = [torch.empty((sa.height, sa.width, 4), dtype=torch.float32, device="cuda") for _ in range(2)]
        R.blend_timesteps(0, 1, 0.3, 10, stream=ctypes.c_void_p(bl.cuda_stream))
        R.upload_timestep_device(0, dev[0].data_ptr(), sc.dims, 3, 1, dev[1].data_ptr(), fsize=tuple(float(f) for f in sc.fsize),
                                 stream=ctypes.c_void_p(up.cuda_stream))
        R.select_timestep(10)
        R.render_device(outs[0].data_ptr(), None, ctypes.c_void_p(rend.cuda_stream))
        R.select_timestep(0)
        R.render_device(outs[1].data_ptr(), None, ctypes.c_void_p(rend.cuda_stream))
        torch.cuda.synchronize()                    # the three streams: read-back
        same(outs[0].cpu().numpy(), want_mid, "the blend of the old step 0")
        same(outs[1].cpu().numpy(), want_c, "the new step 0")
    finally:
        R.close()


# ---- 7. shadows, and the perturbed fetch

@pytest.mark.parametrize("mode", ["shadow", "pert"])
def test_shadows_and_perturbation_on_a_blended_step(gpu_renderer_factory, mode):
    scs = [T.scene(*v, pert=(mode == "pert")) for v in (T.step("f32", 1), T.step("f32", 2), T.blended("f32", 1, 2, 0.3))]
    if mode == "shadow":
        for s in scs:
            s.shadow = (64, 0.75)
    want = fresh_frame(gpu_renderer_factory, scs[2])
    R = ring(gpu_renderer_factory, scs[0], scs[1])
    try:
        R.render()
        R.blend_timesteps(0, 1, 0.3, 10)
        R.select_timestep(10)
        same(R.render(), want, mode)
    finally:
        R.close()


# ---- 8. shards

@pytest.mark.parametrize("shadow", [False, True])
def test_shards_blend_their_regions(gpu_renderer_factory, shadow):
    from _scenes import push_scene
    scs = [T.scene(*v) for v in (T.step("f32", 1), T.step("f32", 2), T.blended("f32", 1, 2, 0.3))]
    if shadow:
        for s in scs:
            s.shadow = (64, 0.75)
    halo = 1
    if shadow:                                      # the halo a frame with shadows needs on these shards
        probe = gpu_renderer_factory()
        try:
            probe.set_shard(0, 2)
            push_scene(probe, scs[0])
            halo = max(probe.shadow_margin()[1], 1)
        finally:
            probe.close()

    def shards(sc):
        rs = []
        for r in range(2):
            R = gpu_renderer_factory()
            rs.append(R)
            R.set_shard(r, 2)
            R.set_option("halo", halo)
            R.set_option("slab_split", 1)           # (frames of different histories: no measured depth cuts)
            push_scene(R, sc)
        return rs
    fresh = shards(scs[2])
    try:
        want = _merged(fresh, scs[2], shadow)
    finally:
        for R in fresh:
            R.close()
    rs = shards(scs[0])
    try:
        _merged(rs, scs[0], shadow)
        for R in rs:
            R.set_timestep_cache(3)
            upload(R, 1, scs[1])
            R.blend_timesteps(0, 1, 0.3, 10)
            R.select_timestep(10)
        same(_merged(rs, scs[2], shadow), want, "merged")
        assert all(R.stat("slab_failures") == 0 for R in rs)
    finally:
        for R in rs:
            R.close()


# ---- 9. the host adapter

def _frames(prefix, n):
    return [np.fromfile("%s.%d.f32" % (prefix, k), np.float32) for k in range(n)]


def test_host_adapter_shows_fractional_time(tmp_path):
    """tests/host/tblend_main drives HipVolumeRenderable::setTimeFraction over a 3-step series; its frames are the ones the C
    ABI gives when the blend is made behind the adapter's back, and the ones of the restated blends drawn alone"""
    exe = os.path.join(ROOT, "tests", "host", "tblend_main")
    alone = os.path.join(ROOT, "tests", "host", "timestep_main")
    for e in (exe, alone):
        assert os.path.exists(e), "%s is not built: __graft_entry__.build() builds it" % e
    steps = [np.ascontiguousarray(T.step("u8", s)[0][..., 0]) for s in (1, 2, 3)]
    d = tmp_path / "series"
    d.mkdir()
    trex = write_series(str(d), steps, shape=(32, 32, 32), tstart=0, cache=3)

    def run(mode, seq, name, trex=trex, d=d):
        p = subprocess.run([exe, mode, trex, "48", "48", "1", seq, str(d / name)], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        counts = [int(line.rsplit("=", 1)[1]) for line in p.stdout.splitlines() if line.startswith("frame ")]
        return _frames(str(d / name), len(counts)), counts, p.stderr
    got, counts, err = run("frac", "0:0,0:0.3,0:0.3,0:0.7,1:0.7,2:0.7", "frac")
    ref, _, _ = run("abi", "0:0,0:0.3,0:0.7,1:0.7,2:0", "abi")
    assert not np.array_equal(ref[0], ref[1]) and not np.array_equal(ref[1], ref[2]) and not np.array_equal(ref[2], ref[3])
    for k, r in enumerate((0, 1, 1, 2, 3, 4)):      # (the last: step 3 does not exist, the frame stays on the whole step 2)
        same(got[k], ref[r], "draw %d" % k)
    assert counts == [0, 1, 1, 2, 3, 3]             # the second 0.3 made no blend, the refused one is not one
    assert "not cached" in err
    # a series that keeps one step resident has nothing to blend with: said once, the frame is the whole step's
    one = tmp_path / "one"
    one.mkdir()
    trex1 = write_series(str(one), steps, shape=(32, 32, 32), tstart=0, cache=1)
    got1, counts1, err1 = run("frac", "0:0,0:0.3,0:0.3", "frac", trex1, one)
    same(got1[1], got1[0], "one resident step")
    same(got1[0], got[0], "step 0")
    assert counts1 == [0, 0, 0] and err1.count("not cached") == 1
    # ... and the restated blends, each drawn alone by a fresh renderer
    def blend8(a, b, w):
        return T.blend(steps[a][..., None], None, steps[b][..., None], None, w)[0][..., 0]
    e = tmp_path / "restated"
    e.mkdir()
    trex2 = write_series(str(e), [blend8(0, 1, 0.3), blend8(0, 1, 0.7), blend8(1, 2, 0.7)], shape=(32, 32, 32), tstart=0, cache=1)
    for t, k in enumerate((1, 3, 4)):
        p = subprocess.run([alone, "draw", trex2, "48", "48", "1", str(t), str(e / ("only%d" % t)), "only=%d" % t],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        same(got[k], np.fromfile(str(e / ("only%d.0.f32" % t)), np.float32), "restated blend %d" % t)
