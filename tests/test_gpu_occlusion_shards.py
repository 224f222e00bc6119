"""Occluded frames on shards (smk.h smk_render_occluded_device with smk_set_shard): every rank reads the same full-window
scene depth, and the merged occluded frame equals the unsharded occluded frame -- RGBA within the sort-last tolerance,
depth bit for bit -- through the in-process exchange, and with shadows through the light exchange."""
import numpy as np
import pytest

from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu
TOL = 2e-5


def _scene_depth(R, sc, seed):
    """a sphere in front of a tilted back wall, plus noise, across the volume's depth range (view depths)"""
    rc = R.raycoef()
    pd = (rc.tau0 + np.arange(rc.nplanes, dtype=np.float64) * rc.dtau) * sc.znear
    h, w = sc.height, sc.width
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((x - 0.4 * w) ** 2 + (y - 0.5 * h) ** 2) / (0.3 * min(w, h)) ** 2
    span = pd[-1] - pd[0]
    wall = pd[0] + span * (0.4 + 0.5 * x / w)
    d = np.where(r2 < 1, pd[len(pd) // 2] - 0.5 * span * np.sqrt(np.clip(1 - r2, 0, 1)), wall)
    d += np.random.default_rng(seed).normal(0, 0.03 * span, d.shape)
    return d.astype(np.float32)


def _not_vacuous(ref, d):
    fin = np.isfinite(d)
    assert ref[..., 3].max() > 0.05 and fin.mean() >= 0.1 and (~fin).mean() >= 0.1, f"vacuous frame: {fin.mean():.3f} finite"


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_occluded_frame_equals_whole(gpu_renderer_factory, smk, world, blend, kernel):
    import torch
    sc = make_scene("cfg3", n=32, size=45, steps=48, pose="rot", f32=True, shade=1)
    npix = sc.width * sc.height
    W = gpu_renderer_factory()
    rs, xs = [], []
    try:
        push_scene(W, sc)
        W.set_blend(blend)
        W.set_option("kernel", kernel)
        zs = _scene_depth(W, sc, 3 + world)
        ref, rd = W.render(depth=True, scene_depth=zs)
        assert W.last_frame_info()[0] == kernel
        _not_vacuous(ref, rd)
        assert not np.array_equal(ref, W.render())
        for r in range(world):
            R = gpu_renderer_factory()
            rs.append(R)
            R.set_shard(r, world)
            push_scene(R, sc)
            R.set_blend(blend)
            R.set_option("kernel", kernel)
            xs.append(smk.binding.Exchange(R, r, world, npix))
        smk.binding.Exchange.connect_local(xs)
        dzs = torch.from_numpy(zs).cuda()
        frame = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        depth = torch.zeros((npix,), dtype=torch.float32, device="cuda")
        for x in xs:
            assert x.partial_depth(0)
        torch.cuda.synchronize()
        for R, x in zip(rs, xs):
            x.acquire(0)
            R.render_device(x.partial(0), x.partial_depth(0), None, d_scene_depth=dzs.data_ptr())
            x.rendered(0)
        smk.binding.Exchange.frame_local_depth(xs, 0, frame.data_ptr(), depth.data_ptr())
        xs[0].wait(None)
        torch.cuda.synchronize()
        for R in rs:
            assert R.stat("slab_failures") == 0
            assert R.last_frame_info()[0] == kernel
        got = frame.cpu().numpy().reshape(sc.height, sc.width, 4)
        gd = depth.cpu().numpy().reshape(sc.height, sc.width)
        assert np.array_equal(gd, rd), f"merged depth differs on {int((gd != rd).sum())} pixels"
        assert np.abs(got - ref).max() <= TOL, f"max abs err {np.abs(got - ref).max()}"
    finally:
        for x in xs:
            x.close()
        for R in rs:
            R.close()
        W.close()


def _shadow_shards(factory, sc, world):
    """P shard contexts, each with the halo its frame with shadows needs (smk_get_shadow_margin)"""
    rs = []
    try:
        for r in range(world):
            R = factory()
            R.set_shard(r, world)
            push_scene(R, sc)
            need = R.shadow_margin()[1]
            R.close()
            R = factory()
            R.set_shard(r, world)
            R.set_option("halo", need)
            push_scene(R, sc)
            rs.append(R)
    except Exception:
        for R in rs:
            R.close()
        raise
    return rs


@pytest.mark.parametrize("f32,shade,light", [(True, 1, (3, 4, -3)), (False, 0, (-2, 3, 4))])
def test_sharded_occluded_shadow_frame_equals_whole(gpu_renderer_factory, smk, f32, shade, light):
    from simian_spacemonkey_amd import sortlast
    sc = make_scene("cfg3", f32=f32, shade=shade, pose="rot")
    sc.light_pos = light
    sc.shadow = (64, 0.75)
    W = gpu_renderer_factory()
    rs = []
    try:
        push_scene(W, sc)
        zs = _scene_depth(W, sc, 17)
        ref, rd = W.render(depth=True, scene_depth=zs)
        _not_vacuous(ref, rd)
        assert not np.array_equal(ref, W.render())
        rs = _shadow_shards(gpu_renderer_factory, sc, 2)
        got, gd = sortlast.render_shadow_frame_local(rs, depth=True, scene_depth=zs)
        got, gd = got.cpu().numpy(), gd.cpu().numpy()
        assert np.array_equal(gd, rd), f"merged depth differs on {int((gd != rd).sum())} pixels"
        assert np.abs(got - ref).max() <= TOL, f"max abs err {np.abs(got - ref).max()}"
    finally:
        W.close()
        for R in rs:
            R.close()
