"""The device-resident time-step cache (smk.h: smk_set_timestep_cache, smk_upload_timestep[_device], smk_select_timestep,
smk_get_timesteps).  A frame after a switch must be the frame a fresh context renders from that step alone, bit for bit,
under every ray-marcher and with or without brick flags; the ring keeps the current step, refuses what does not belong to
the series, and the asynchronous upload orders itself against the frames in flight on other streams.  The steps are
distinct volumes: the reference generator's spheres with different seeds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _scenes import make_scene, push_scene, vgh_volume
from _step_gpu import fresh_frame, merged_frame as _merged
from _trex_series import write_series

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (1, 2, 3)


def step_scene(seed, f32=True, kind="cfg3", **kw):
    """the config 3 scene over time step `seed`'s volume"""
    sc = make_scene(kind, n=32, size=64, steps=64, pose="diag", f32=f32, shade=1, **kw)
    vgh8, vghf, nrm = vgh_volume(32, seed)
    sc.data, sc.grad = (vghf if f32 else vgh8), nrm
    return sc


def upload_step(R, t, sc):
    R.upload_timestep(t, sc.data, sc.grad, fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")


def test_steps_are_distinct():
    a, b, c = (vgh_volume(32, s)[0] for s in SEEDS)
    assert not np.array_equal(a, b) and not np.array_equal(b, c) and not np.array_equal(a, c)


@pytest.mark.parametrize("bricks", [0, 1])
@pytest.mark.parametrize("kernel", [0, 1, 2, 3])
@pytest.mark.parametrize("f32", [False, True])
def test_switch_frames_equal_fresh_contexts(gpu_renderer_factory, f32, kernel, bricks):
    scs = [step_scene(s, f32) for s in SEEDS]
    opts = (("kernel", kernel), ("bricks", bricks))
    fresh = [fresh_frame(gpu_renderer_factory, sc, opts) for sc in scs]
    assert not np.array_equal(fresh[0], fresh[1]) and not np.array_equal(fresh[1], fresh[2])
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(3)
        push_scene(R, scs[0])                       # step 0: smk_upload_volume, the current step
        for k, v in opts:
            R.set_option(k, v)
        upload_step(R, 1, scs[1])
        upload_step(R, 2, scs[2])
        assert R.timesteps() == (0, [0, 1, 2])
        for t in (2, 0, 1, 2, 2, 0):
            R.select_timestep(t)
            got = R.render()
            assert np.array_equal(got, fresh[t]), "step %d: max diff %g" % (t, np.abs(got - fresh[t]).max())
            if kernel:
                assert R.last_frame_info()[0] == {1: 1, 2: 2, 3: 4}[kernel]
        assert R.stat("slab_failures") == 0
        if f32 and kernel == 0 and bricks == 1:     # ... and against the CPU checker
            R.select_timestep(1)
            assert np.abs(R.render() - scs[1].render()).max() <= 1e-4
    finally:
        R.close()


@pytest.mark.parametrize("kind", ["cfg3", "tf3d_panes"])
def test_brick_flags_follow_the_step(gpu_renderer_factory, kind):
    scs = [step_scene(s, True, kind) for s in SEEDS]
    want = [fresh_frame(gpu_renderer_factory, sc, render=lambda R: R.brick_flags()[0]) for sc in scs]
    assert not np.array_equal(want[0], want[1])
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(3)
        push_scene(R, scs[0])
        R.render()
        for t in (1, 2):
            upload_step(R, t, scs[t])
        for t in (1, 0, 2):
            R.select_timestep(t)
            assert np.array_equal(R.brick_flags()[0], want[t]), t
            R.render()
    finally:
        R.close()


def test_ring_replacement_and_refusals(gpu_renderer_factory, smk):
    scs = [step_scene(s, True) for s in SEEDS]
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match="at least"):
            R.set_timestep_cache(0)
        R.set_timestep_cache(2)
        push_scene(R, scs[0], upload=False)
        upload_step(R, 0, scs[0])                   # the first step of an empty context becomes current
        assert R.timesteps() == (0, [0])
        upload_step(R, 1, scs[1])
        upload_step(R, 2, scs[2])                   # replaces step 1: the current step 0 is never evicted
        assert R.timesteps() == (0, [0, 2])
        R.select_timestep(2)
        upload_step(R, 1, scs[1])                   # the slot after the last written: step 0's
        assert R.timesteps() == (2, [2, 1])
        with pytest.raises(smk.SmkError, match="not cached"):
            R.select_timestep(0)
        with pytest.raises(smk.SmkError, match="not cached"):
            R.select_timestep(99)
        assert R.timesteps()[0] == 2
        # what does not belong to the series, field named
        v8, vf, nrm = vgh_volume(32, 4)
        fs = tuple(float(f) for f in scs[0].fsize)
        with pytest.raises(smk.SmkError, match="dtype"):
            R.upload_timestep(3, v8, nrm, fsize=fs)
        with pytest.raises(smk.SmkError, match="normals"):
            R.upload_timestep(3, vf, None, fsize=fs)
        with pytest.raises(smk.SmkError, match="nelts"):
            R.upload_timestep(3, np.ascontiguousarray(vf[..., :2]), nrm, fsize=fs)
        with pytest.raises(smk.SmkError, match="datamode"):
            R.upload_timestep(3, vf, nrm, fsize=fs, dmode="V2GH")
        with pytest.raises(smk.SmkError, match="extents"):
            R.upload_timestep(3, vf, nrm, fsize=(1.0, 1.0, 0.5))
        vs = vgh_volume(24, 4)
        with pytest.raises(smk.SmkError, match="sizes"):
            R.upload_timestep(3, vs[1], vs[2])
        assert R.timesteps() == (2, [2, 1])
        got = R.render()
        assert np.array_equal(got, fresh_frame(gpu_renderer_factory, scs[2]))
        # a capacity of one holds only the current step
        R.set_timestep_cache(1)
        assert R.timesteps() == (2, [2])
        with pytest.raises(smk.SmkError, match="one step"):
            upload_step(R, 0, scs[0])
        upload_step(R, 2, scs[1])                   # the current step overwritten in place
        assert np.array_equal(R.render(), fresh_frame(gpu_renderer_factory, scs[1]))
        # smk_upload_volume after a series: one step, today's frame
        R.set_timestep_cache(3)
        upload_step(R, 5, scs[0])
        push_scene(R, scs[2])
        assert R.timesteps() == (2, [2])
        assert np.array_equal(R.render(), fresh_frame(gpu_renderer_factory, scs[2]))
    finally:
        R.close()


def test_asynchronous_upload_beside_frames_in_flight(gpu_renderer_factory):
    import torch
    scs = [step_scene(s, True) for s in SEEDS]
    fresh = [fresh_frame(gpu_renderer_factory, sc) for sc in scs]
    dev = [(torch.from_numpy(np.ascontiguousarray(sc.data)).cuda(), torch.from_numpy(np.ascontiguousarray(sc.grad)).cuda())
           for sc in scs]
    dims = scs[0].dims
    fs = tuple(float(f) for f in scs[0].fsize)
    w, h = scs[0].width, scs[0].height
    up, rend = torch.cuda.Stream(), torch.cuda.Stream()
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(2)
        push_scene(R, scs[0])
        torch.cuda.synchronize()                    # nothing is in flight when the two streams start
        outs, want = [], []

        def frame(t):
            o = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
            outs.append(o)
            want.append(t)
            R.render_device(o.data_ptr(), None, ctypes.c_void_p(rend.cuda_stream))
        for _ in range(16):                          # frames of step 0 in flight ...
            frame(0)
        R.upload_timestep_device(1, dev[1][0].data_ptr(), dims, 3, 1, dev[1][1].data_ptr(), fsize=fs,
                                 stream=ctypes.c_void_p(up.cuda_stream))   # ... while step 1 goes up on another stream
        R.select_timestep(1)
        for _ in range(4):
            frame(1)
        # step 2 takes step 0's slot, which the first 16 frames read: the upload waits for them
        R.upload_timestep_device(2, dev[2][0].data_ptr(), dims, 3, 1, dev[2][1].data_ptr(), fsize=fs,
                                 stream=ctypes.c_void_p(up.cuda_stream))
        for _ in range(4):
            frame(1)
        R.select_timestep(2)
        for _ in range(4):
            frame(2)
        R.select_timestep(1)
        frame(1)
        torch.cuda.synchronize()                    # both streams: read-back
        for i, (o, t) in enumerate(zip(outs, want)):
            got = o.cpu().numpy()
            assert np.array_equal(got, fresh[t]), "frame %d (step %d): max diff %g" % (i, t, np.abs(got - fresh[t]).max())
        assert R.stat("slab_failures") == 0
    finally:
        R.close()


@pytest.mark.parametrize("mode", ["shadow", "pert"])
def test_shadows_and_perturbation_after_a_switch(gpu_renderer_factory, mode):
    scs = [step_scene(s, True, pert=(mode == "pert")) for s in SEEDS[:2]]
    if mode == "shadow":
        for sc in scs:
            sc.shadow = (64, 0.75)
    want = fresh_frame(gpu_renderer_factory, scs[1])
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(2)
        push_scene(R, scs[0])
        R.render()
        upload_step(R, 1, scs[1])
        R.select_timestep(1)
        got = R.render()
        assert np.array_equal(got, want), np.abs(got - want).max()
    finally:
        R.close()


@pytest.mark.parametrize("shadow", [False, True])
def test_shards_switch_and_merge(gpu_renderer_factory, shadow):
    scs = [step_scene(s, True) for s in SEEDS[:2]]
    if shadow:
        for sc in scs:
            sc.shadow = (64, 0.75)
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
    fresh = shards(scs[1])
    try:
        want = _merged(fresh, scs[1], shadow)
    finally:
        for R in fresh:
            R.close()
    rs = shards(scs[0])
    try:
        _merged(rs, scs[0], shadow)
        for R in rs:
            R.set_timestep_cache(2)
            upload_step(R, 1, scs[1])
            R.select_timestep(1)
        got = _merged(rs, scs[1], shadow)
        assert np.array_equal(got, want), np.abs(got - want).max()
        assert all(R.stat("slab_failures") == 0 for R in rs)
    finally:
        for R in rs:
            R.close()


def test_host_adapter_follows_the_time_step(tmp_path):
    """tests/host/timestep_main drives HipVolumeRenderable through a 3-step .trex series as the key handler does; every
    draw() shows the step gluvv.volren.timestep names (before this, every step rendered the one uploaded first)"""
    exe = os.path.join(ROOT, "tests", "host", "timestep_main")
    assert os.path.exists(exe), "tests/host/timestep_main is not built: __graft_entry__.build() builds it"
    steps = [np.ascontiguousarray(vgh_volume(32, s)[0][..., 0]) for s in SEEDS]
    for cache in (1, 3):
        d = tmp_path / ("c%d" % cache)
        d.mkdir()
        trex = write_series(str(d), steps, shape=(32, 32, 32), tstart=0, cache=cache)
        seq = [0, 1, 2, 1, 0, 2]
        p = subprocess.run([exe, "draw", trex, "48", "48", "1", ",".join(map(str, seq)), str(d / "seq")],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        alone = []
        for t in range(3):
            p = subprocess.run([exe, "draw", trex, "48", "48", "1", str(t), str(d / ("only%d" % t)), "only=%d" % t],
                               capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, p.stderr
            alone.append(np.fromfile(str(d / ("only%d.0.f32" % t)), np.float32))
        assert not np.array_equal(alone[0], alone[1]) and not np.array_equal(alone[1], alone[2])
        for k, t in enumerate(seq):
            got = np.fromfile(str(d / ("seq.%d.f32" % k)), np.float32)
            assert np.array_equal(got, alone[t]), "cache %d, draw %d (step %d): max diff %g" % (cache, k, t, np.abs(got - alone[t]).max())
