"""First-hit depth on frames with half-angle shadows (smk.h smk_set_shadow): the view depth of the nearest
sample the eye pass composites along the pixel's half-angle ray.  Both ray-marchers and the launch-per-slice form agree bit
for bit, the RGBA does not change with the request, the depth lands on a known surface, and the depth merged from shards
with shadows equals the unsharded frame's exactly."""
import numpy as np
import pytest

import oracle as O
from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu

LIGHTS = {"eye_side": (0, 0, -5), "oblique": (3, 4, -3), "behind": (-2, 3, 4), "side": (5, 1, 0.5)}


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def _not_vacuous(d):
    assert np.isfinite(d).mean() >= 0.1, f"vacuous depth: {np.isfinite(d).mean():.3f} finite"


@pytest.mark.parametrize("light", sorted(LIGHTS))
@pytest.mark.parametrize("kind,f32,shade,pose", [("cfg3", True, 1, "rot"), ("cfg3", False, 1, "diag"), ("tf3d", False, 0, "back"),
                                                 ("cfg4", True, 1, "side")])
def test_shadow_depth_on_every_path(R, light, kind, f32, shade, pose):
    """gather kernel, slice-ring kernel, a launch per slice (option shadow_march 0) and all slices in one cooperative launch
    (option shadow_fused): depth bit-identical, whichever way the slices run; the RGBA of render(depth=True) is
    bit-identical to render()'s."""
    sc = make_scene(kind, n=48, size=112, steps=150, f32=f32, shade=shade, pose=pose)
    sc.light_pos = LIGHTS[light]
    sc.shadow = (96, 0.7)
    push_scene(R, sc)
    out = {}
    try:
        for kern in (1, 2):
            R.set_option("kernel", kern)
            out[kern] = R.render(depth=True)
            assert R.last_frame_info()[0] == kern
            assert np.array_equal(out[kern][0], R.render())
        R.set_option("kernel", 0)
        R.set_option("shadow_march", 0)
        out[3] = R.render(depth=True)
        assert R.last_frame_info()[0] == 3
        assert np.array_equal(out[3][0], R.render())
        R.set_option("shadow_march", 1)
        R.set_option("shadow_fused", 1)      # (all slices in one cooperative launch: the same per-slice arithmetic)
        out[4] = R.render(depth=True)
        assert R.last_frame_info()[0] == 3
        assert np.array_equal(out[4][0], out[3][0])
    finally:
        R.set_option("shadow_fused", 0)
        R.set_option("shadow_march", 1)
        R.set_option("kernel", 0)
    d1 = out[1][1]
    _not_vacuous(d1)
    assert np.array_equal(d1, out[2][1]), "gather vs slice-ring depth"
    assert np.array_equal(d1, out[3][1]), "two marches vs a launch per slice: depth"
    assert np.array_equal(d1, out[4][1]), "two marches vs the cooperative launch: depth"
    # a pixel has a depth exactly where its frame has colour
    assert np.array_equal(np.isfinite(d1), out[1][0][..., 3] > 0)


def _plane_scene(z0, pose_deg):
    """u8 volume transparent below voxel plane z0 and opaque from it on: values 0 / 255, a 2-D table whose alpha is 0 only
    at value 0 -- the first hit of every ray that reaches the plane from the transparent side lies on it"""
    n = 32
    v = np.zeros((n, n, n, 3), np.uint8)
    v[z0:, :, :, 0] = 255
    sc = O.Scene(v)
    tex = np.zeros((256, 256, 4), np.uint8)
    tex[:, 1:] = (200, 150, 100, 255)
    sc.tf_vg = tex
    sc.tf_mode = 1
    sc.width = sc.height = 80
    sc.steps = 96
    sc.xform = O.rotation((1, 1, 0), pose_deg)
    sc.shade_mode = 0
    return sc


@pytest.mark.parametrize("light", ["oblique", "behind"])
@pytest.mark.parametrize("z0,pose_deg", [(12, 20), (20, -35)])
def test_half_angle_depth_lands_on_the_surface(R, light, z0, pose_deg):
    """An independent check of the half-angle depth: on the plane volume the unshadowed depth (parity-tested against the CPU
    checker, tests/test_gpu_slab.py) and the shadowed one each lie within one slice spacing of the surface along the pixel's
    ray -- the view-aligned planes' spacing in view depth is rc.dis, the half-angle slices' is |dtau| * znear, dtau =
    dnum / nD -- so they agree within the sum of the two on every pixel."""
    sc = _plane_scene(z0, pose_deg)
    push_scene(R, sc)
    plain, pd = R.render(depth=True)
    dis = R.raycoef().dis
    sc.light_pos = LIGHTS[light]
    sc.shadow = (64, 0.75)
    push_scene(R, sc, upload=False)
    try:
        for kern in (1, 2):
            R.set_option("kernel", kern)
            rgba, sd = R.render(depth=True)
            assert R.last_frame_info()[0] == kern
            c = R.shadowcoef()
            px = (np.arange(sc.width, dtype=np.float64) + 0.5) * c.pxs + c.pxl
            py = (np.arange(sc.height, dtype=np.float64) + 0.5) * c.pys + c.pyl
            nD = px[None, :] * c.nDx + py[:, None] * c.nDy + c.nDc
            step = np.abs(c.dnum / nD) * sc.znear
            both = np.isfinite(pd) & np.isfinite(sd)
            # (the two slice sets can disagree about a ray that only grazes the volume's silhouette)
            assert both.mean() > 0.5 and (np.isfinite(pd) != np.isfinite(sd)).mean() < 0.02
            err = np.abs(sd[both].astype(np.float64) - pd[both])
            bound = (step + dis)[both]
            assert (err <= bound).all(), f"kernel {kern}: worst |shadowed - plain| / bound = {(err / bound).max():.3f}"
            # (the shadowed depth is not the plain one: it is placed on other slices)
            assert not np.array_equal(sd, pd)
    finally:
        R.set_option("kernel", 0)


LIGHTS_SH = dict(LIGHTS, low=(-4, -2, -3))
SHARD_CASES = [
    (2, "cfg3", False, 1, "rot", "oblique"),
    (4, "cfg3", True, 1, "rot", "low"),
    (4, "tf3d", False, 0, "rot", "side"),
    (8, "cfg3", True, 1, "rot", "eye_side"),
    (8, "cfg3", False, 0, "side", "behind"),
]


def _shards(factory, sc, world):
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


@pytest.mark.parametrize("case", SHARD_CASES, ids=["-".join(str(x) for x in c) for c in SHARD_CASES])
def test_sharded_shadow_depth_equals_whole(gpu_renderer_factory, smk, case):
    """P shard contexts with shadows, merged through render_shadow_frame_local(depth=True): the depth equals the unsharded
    shadowed frame's exactly, while the RGBA stays within the sharded-shadow tolerance of tests/test_gpu_shadow_shards.py."""
    from simian_spacemonkey_amd import sortlast
    world, kind, f32, shade, pose, light = case
    sc = make_scene(kind, f32=f32, shade=shade, pose=pose)
    sc.light_pos = LIGHTS_SH[light]
    sc.shadow = (64, 0.75)
    W = gpu_renderer_factory()
    rs = []
    try:
        push_scene(W, sc)
        ref, rd = W.render(depth=True)
        _not_vacuous(rd)
        rs = _shards(gpu_renderer_factory, sc, world)
        got, gd = sortlast.render_shadow_frame_local(rs, depth=True)
        got, gd = got.cpu().numpy(), gd.cpu().numpy()
        assert np.array_equal(gd, rd), f"merged depth differs on {int((gd != rd).sum())} pixels"
        assert np.abs(got - ref).max() <= 2e-5
        # the RGBA-only form is unchanged
        assert np.array_equal(sortlast.render_shadow_frame_local(rs).cpu().numpy(), got)
    finally:
        W.close()
        for R in rs:
            R.close()
