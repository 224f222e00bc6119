"""The clip-plane widget's data slice on shards (smk.h smk_set_clip_slice with smk_set_shard): every rank draws the part of
the quad whose hit points lie in its own region, composed with its own volume frame, before the exchange -- and the
merged frame equals the unsharded frame with the slice, within the sort-last tolerance, for a plane that crosses the
shard boundaries and for one that lies exactly on the x split, before and after passes.

The pass is the one the geometry calls for -- before when the eye looks at the kept side of the plane, after when it looks
at the cut face -- as it is for the reference's dv: per-rank drawing rests on everything beyond (before) or in front of
(after) the slice being clipped away (smk.h)."""
import numpy as np
import pytest

from _clip_slice_cases import PASS_TABLE, clip_vpos, widget_corners
from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu
TOL = 2e-5      # tests/test_gpu_occlusion_shards.py's
ALPHA = 0.6
# (oaxis, plane position as a fraction of fSize): a z plane crosses the x and y splits; x planes at 0.5 lie on the x split,
# the quad 0.001 beyond it on either side
PLANES = {"crossing": (5, 0.45), "on_split_x+": (1, 0.5), "on_split_x-": (2, 0.5)}


PASSES_SEEN = set()


def _geometric_pass(sc, oaxis, vpos):
    """2 (after) when the eye, in volume space, lies on the side of the plane that is cut away, else 1 (before)"""
    M = np.array(sc.mv(), np.float64).reshape(4, 4).T
    eye = np.linalg.inv(M)[:3, 3]
    a = (oaxis - 1) // 2
    keeps_low = (oaxis - 1) % 2 == 0            # X+ Y+ Z+ keep coordinate <= vpos (smk.h smk_set_clip)
    return 2 if (eye[a] > vpos[a]) == keeps_low else 1


# poses with the eye on either side of each plane: "back" looks at the z plane from behind, "x-" at the x planes from -x
CASES = [("crossing", "rot"), ("crossing", "back"), ("on_split_x+", "rot"), ("on_split_x+", "x-"), ("on_split_x-", "rot"),
         ("on_split_x-", "x-")]


@pytest.mark.parametrize("plane,pose", CASES)
@pytest.mark.parametrize("world", [2, 4, 8])
def test_sharded_frame_with_slice_equals_whole(gpu_renderer_factory, smk, world, plane, pose):
    import torch
    oaxis, frac = PLANES[plane]
    sc = make_scene("cfg3", n=32, size=45, steps=48, pose=pose, f32=True, shade=1)
    vpos = clip_vpos(oaxis, sc.fsize, frac)
    sc.clip = (oaxis, vpos)
    corners = widget_corners(oaxis, vpos, sc.fsize)
    want_pass = _geometric_pass(sc, oaxis, vpos)
    dv = -0.5 if PASS_TABLE[oaxis][0] == want_pass else 0.5
    PASSES_SEEN.add((plane, want_pass))
    npix = sc.width * sc.height
    W = gpu_renderer_factory()
    rs, xs = [], []
    try:
        push_scene(W, sc)
        W.set_option("kernel", 1)
        plain = W.render()
        W.set_clip_slice(corners, ALPHA, dv, "r8k")
        ref = W.render()
        assert W.stat("clip_slice_pass") == want_pass
        assert plain[..., 3].max() > 0.05 and (np.abs(ref - plain).max(axis=-1) > 1e-3).sum() > 100, "vacuous"
        for r in range(world):
            R = gpu_renderer_factory()
            rs.append(R)
            R.set_shard(r, world)
            push_scene(R, sc)
            R.set_option("kernel", 1)
            R.set_clip_slice(corners, ALPHA, dv, "r8k")
            xs.append(smk.binding.Exchange(R, r, world, npix))
        smk.binding.Exchange.connect_local(xs)
        frame = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for R, x in zip(rs, xs):
            x.acquire(0)
            R.render_device(x.partial(0), None, None)
            x.rendered(0)
        smk.binding.Exchange.frame_local(xs, 0, frame.data_ptr())
        xs[0].wait(None)
        torch.cuda.synchronize()
        for R in rs:
            assert R.stat("clip_slice_pass") == want_pass
        got = frame.cpu().numpy().reshape(sc.height, sc.width, 4)
        err = np.abs(got - ref).max()
        print("world %d %s %s pass %d: merged vs unsharded max abs err %.3g" % (world, plane, pose, want_pass, err))
        assert err <= TOL, f"max abs err {err}"
    finally:
        for x in xs:
            x.close()
        for R in rs:
            R.close()
        W.close()


def test_both_passes_were_merged():
    """(runs after the cases above) every plane was drawn before and after the volume"""
    assert PASSES_SEEN == {(p, k) for p in PLANES for k in (1, 2)}, PASSES_SEEN


def test_after_pass_under_gl_max_is_refused_on_shards(gpu_renderer_factory, smk):
    """a maximum cannot merge `slice over volume`: the frame fails with the reason instead of merging to something else"""
    oaxis = 1
    sc = make_scene("cfg3", n=32, size=45, steps=48, pose="rot", f32=True, shade=1)
    vpos = clip_vpos(oaxis, sc.fsize)
    sc.clip = (oaxis, vpos)
    R = gpu_renderer_factory()
    try:
        R.set_shard(0, 2)
        push_scene(R, sc)
        R.set_option("kernel", 1)
        R.set_blend(2)
        R.set_clip_slice(widget_corners(oaxis, vpos, sc.fsize), ALPHA, 0.5, "r8k")
        with pytest.raises(smk.SmkError, match="SMK_BLEND_MAX"):
            R.render()
        R.set_clip_slice(widget_corners(oaxis, vpos, sc.fsize), ALPHA, -0.5, "r8k")
        assert R.render() is not None and R.stat("clip_slice_pass") == 1
    finally:
        R.close()
