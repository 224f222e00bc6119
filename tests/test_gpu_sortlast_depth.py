"""First-hit depth through the sort-last merge (smk.h smk_composite_over_depth_device, smk_exchange_partial_depth,
smk_exchange_frame[_local]_depth).  The merged depth of a pixel is the minimum over the ranks' depths and
equals the unsharded frame's bit for bit, in every blend mode, on both ray-marchers; the merged RGBA is what the RGBA-only
merge delivers."""
import ctypes

import numpy as np
import pytest

from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu
TOL = 2e-5
POSES = ("rot", "back", "side")


def _scene(pose):
    return make_scene("cfg3", n=32, size=45, steps=48, pose=pose, f32=True, shade=1)


def _not_vacuous(d):
    fin = np.isfinite(d)
    assert fin.mean() >= 0.1 and (~fin).mean() >= 0.1, f"vacuous depth: {fin.mean():.3f} finite"


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("world", [2, 4, 8])
def test_exchange_in_process_carries_depth(gpu_renderer_factory, smk, world, blend, kernel):
    """`world` shard contexts of this process render three frames (three poses) in flight through both slots of the
    in-process exchange, RGBA and depth; the merged depth equals the unsharded context's exactly (+inf included), the
    merged RGBA is within the sort-last tolerance.  An odd pixel count leaves the last tile short."""
    import torch
    scs = [_scene(p) for p in POSES]
    npix = scs[0].width * scs[0].height
    W = gpu_renderer_factory()
    rs, xs = [], []
    try:
        push_scene(W, scs[0])
        W.set_blend(blend)
        W.set_option("kernel", kernel)
        refs = []
        for sc in scs:
            push_scene(W, sc, upload=False)
            refs.append(W.render(depth=True))
            assert W.last_frame_info()[0] == kernel
        for r in range(world):
            R = gpu_renderer_factory()
            rs.append(R)
            R.set_shard(r, world)
            push_scene(R, scs[0])
            R.set_blend(blend)
            R.set_option("kernel", kernel)
            xs.append(smk.binding.Exchange(R, r, world, npix))
        smk.binding.Exchange.connect_local(xs)
        for x in xs:
            assert x.partial_depth(0) and x.partial_depth(1)
        frames = torch.zeros((len(scs), npix, 4), dtype=torch.float32, device="cuda")
        depths = torch.zeros((len(scs), npix), dtype=torch.float32, device="cuda")
        for i, sc in enumerate(scs):
            slot = i & 1
            for R, x in zip(rs, xs):
                push_scene(R, sc, upload=False)
                x.acquire(slot)
                R.render_device(x.partial(slot), x.partial_depth(slot), None)
                x.rendered(slot)
            smk.binding.Exchange.frame_local_depth(xs, slot, frames[i].data_ptr(), depths[i].data_ptr())
        xs[0].wait(None)
        torch.cuda.synchronize()
        for R in rs:
            assert R.stat("slab_failures") == 0
            assert R.last_frame_info()[0] == kernel
        for i, sc in enumerate(scs):
            ref, rd = refs[i]
            got = frames[i].cpu().numpy().reshape(sc.height, sc.width, 4)
            gd = depths[i].cpu().numpy().reshape(sc.height, sc.width)
            _not_vacuous(rd)
            assert np.array_equal(gd, rd), f"frame {i}: merged depth differs from the unsharded frame's"
            assert ref[..., 3].max() > 0.05 and np.abs(got - ref).max() <= TOL, i
    finally:
        for x in xs:
            x.close()
        for R in rs:
            R.close()
        W.close()


@pytest.mark.parametrize("blend", [0, 2])
@pytest.mark.parametrize("nlayers", [1, 3, 8])
def test_composite_over_depth_against_numpy(gpu_renderer_factory, blend, nlayers):
    """The merge with depth against a numpy restatement: ordered over (or per-component max) of the RGBA layers, minimum of
    the depth layers; its RGBA is bit-identical to smk_composite_over_device's on the same layers."""
    import torch
    R = gpu_renderer_factory()
    try:
        R.set_blend(blend)
        npix = 1000 + 37
        g = np.random.default_rng(7 + nlayers)
        a = g.uniform(0, 1, (nlayers, npix)).astype(np.float32)
        a[g.uniform(size=a.shape) < 0.4] = 0
        rgba = np.concatenate([g.uniform(0, 1, (nlayers, npix, 3)).astype(np.float32) * a[..., None], a[..., None]], -1)
        dep = g.uniform(0.5, 3.0, (nlayers, npix)).astype(np.float32)
        dep[a == 0] = np.inf
        order = list(g.permutation(nlayers))
        L = torch.from_numpy(rgba).cuda()
        D = torch.from_numpy(dep).cuda()
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        out_plain = torch.zeros_like(out)
        dout = torch.zeros((npix,), dtype=torch.float32, device="cuda")
        R.composite_over_depth_device(L.data_ptr(), D.data_ptr(), nlayers, order, npix, out.data_ptr(), dout.data_ptr())
        R.composite_over_device(L.data_ptr(), nlayers, order, npix, out_plain.data_ptr())
        torch.cuda.synchronize()
        got, gd = out.cpu().numpy(), dout.cpu().numpy()
        assert np.array_equal(got, out_plain.cpu().numpy())
        assert np.array_equal(gd, dep.min(0))
        acc = np.zeros((npix, 4), np.float64)
        for l in order:
            acc = np.maximum(acc, rgba[l]) if blend == 2 else acc + (1.0 - acc[:, 3:4]) * rgba[l]
        assert np.abs(got - acc).max() <= 1e-6
    finally:
        R.close()


def _have_rccl():
    for n in ("librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"):
        try:
            ctypes.CDLL(n)
            return True
        except OSError:
            pass
    return False


def test_exchange_rccl_transport_carries_depth_at_world_one(gpu_renderer_factory, smk):
    """The RCCL transport with depth on what one GPU allows: the frame and its depth pass through smk_exchange_frame_depth
    unchanged (no peer: the own tile is merged and delivered)."""
    import torch
    if not _have_rccl():
        pytest.skip("librccl is not installed")
    sc = _scene("rot")
    npix = sc.width * sc.height
    R = gpu_renderer_factory()
    x = None
    try:
        R.set_shard(0, 1)
        push_scene(R, sc)
        ref, rd = R.render(depth=True)
        _not_vacuous(rd)
        x = smk.binding.Exchange(R, 0, 1, npix, id=smk.binding.exchange_unique_id())
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        dout = torch.zeros((npix,), dtype=torch.float32, device="cuda")
        R.render_device(x.partial(0), x.partial_depth(0), None)
        x.rendered(0)
        x.frame_depth(0, out.data_ptr(), dout.data_ptr())
        x.wait(None)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(sc.height, sc.width, 4), ref)
        assert np.array_equal(dout.cpu().numpy().reshape(sc.height, sc.width), rd)
    finally:
        if x is not None:
            x.close()
        R.close()


def test_depth_requests_follow_the_exchange(gpu_renderer_factory, smk):
    """A depth frame from an exchange that never enabled depth is refused with the reason, and so is an RGBA-only frame
    from one that did, or in-process ranks that disagree."""
    import torch
    sc = _scene("rot")
    npix = sc.width * sc.height
    rs, xs = [], []
    try:
        for r in range(2):
            R = gpu_renderer_factory()
            rs.append(R)
            R.set_shard(r, 2)
            push_scene(R, sc)
            xs.append(smk.binding.Exchange(R, r, 2, npix))
        smk.binding.Exchange.connect_local(xs)
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        dout = torch.zeros((npix,), dtype=torch.float32, device="cuda")
        with pytest.raises(smk.SmkError, match="carries no depth"):
            smk.binding.Exchange.frame_local_depth(xs, 0, out.data_ptr(), dout.data_ptr())
        xs[1].partial_depth(0)
        with pytest.raises(smk.SmkError, match="all or none"):
            smk.binding.Exchange.frame_local_depth(xs, 0, out.data_ptr(), dout.data_ptr())
        xs[0].partial_depth(0)
        with pytest.raises(smk.SmkError, match="carries depth"):
            smk.binding.Exchange.frame_local(xs, 0, out.data_ptr())
        with pytest.raises(smk.SmkError, match="no depth buffer"):
            smk.binding.Exchange.frame_local_depth(xs, 0, out.data_ptr(), None)
        torch.cuda.synchronize()
    finally:
        for x in xs:
            x.close()
        for R in rs:
            R.close()
