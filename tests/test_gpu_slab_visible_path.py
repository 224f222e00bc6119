"""The visible path of the slice-ring kernel's consumers.  Under the separable (value, gradient) table a lane whose
occupancy bit is set issues its table loads and then runs the normal's share of the Phong term -- the second batch of
LDS reads, the interpolation, smk_shade_geom -- before it touches a texel; alpha, the third-axis alpha, `hit`, colour,
smk_shade_apply, first-hit depth and the blend follow in their old order.  Only independent work moved, so every
frame must still equal the gather kernel's bit for bit (which shades with the unsplit smk_shade_sample) and the CPU
checker's within the suite's tolerance: with and without brick flags, both voxel types, both Phong forms, the lazy
third channel, lanes that pay the normal work and then turn out transparent, rays that saturate right after a
reordered turn, first-hit depth, and the big workgroups that hold the normals in registers (option "tile")."""
import functools

import numpy as np
import pytest

from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def _scene(kind, shade, f32, pose="diag", variant=None):
    """the scene and the checker's frame of it, made once and shared (never written to)"""
    sc = make_scene(kind, n=32, size=64, steps=64, pose=pose, f32=f32, shade=shade)
    if variant == "h_upper_half_clear":   # third-axis alpha 0 over the upper half of its range
        h = sc.tf_h.copy()
        h[:, h.shape[1] // 2:, 3] = 0
        sc.tf_h = h
    elif variant == "opaque_band":        # alpha 255 on a band of values: rays through it saturate
        t = sc.tf_vg.copy()
        t[:, 96:160] = (200, 120, 40, 255)
        sc.tf_vg = t
    ref = sc.render()
    ref.setflags(write=False)
    return sc, ref


def _gather_and_ring(R, sc, bricks=1, tile=0):
    push_scene(R, sc)
    R.set_option("bricks", bricks)
    try:
        R.set_option("kernel", 1)
        a = R.render()
        R.set_option("kernel", 2)           # forced: raises if the slice-ring kernel does not apply
        R.set_option("tile", tile)
        b = R.render()
        assert R.last_frame_info()[0] == 2
        assert R.stat("slab_status") == 0
    finally:
        R.set_option("tile", 0)
        R.set_option("kernel", 0)
        R.set_option("bricks", 1)
    return a, b


CASES = [("cfg3", 1, True, "diag"), ("cfg3", 1, False, "diag"), ("cfg3", 2, True, "diag"), ("cfg3", 2, False, "diag"),
         ("cfg4", 1, True, "diag"), ("cfg4", 1, False, "diag"), ("cfg2", 0, True, "diag"), ("cfg3", 1, True, "rot")]


@pytest.mark.parametrize("bricks", [0, 1])
@pytest.mark.parametrize("kind,shade,f32,pose", CASES)
def test_slice_ring_equals_gather(R, kind, shade, f32, pose, bricks):
    sc, ref = _scene(kind, shade, f32, pose)
    a, b = _gather_and_ring(R, sc, bricks)
    assert ref[..., 3].max() > 0.05
    assert np.array_equal(a, b), "slice-ring and gather kernels differ: %g" % np.abs(a - b).max()
    assert np.abs(b - ref).max() <= TOL


@functools.lru_cache(maxsize=None)
def _transparent_behind_the_bit(f32):
    """Samples whose (v, g) alpha is not 0 -- so the quad's occupancy bit is set -- while the third-axis alpha is exactly
    0: the checker's frame of the same scene under a third-axis table that is opaque exactly where the scene's own table
    and both neighbouring entries are clear (a lookup that returns anything there interpolates two clear entries)."""
    sc, _ = _scene("cfg4", 1, f32, "diag", "h_upper_half_clear")
    z = sc.tf_h[0, :, 3] == 0
    deep = z & np.concatenate(([True], z[:-1])) & np.concatenate((z[1:], [True]))
    w = sc.tf_h.copy()
    w[:, :, 3] = np.where(deep, 255, 0)[None, :]
    probe = make_scene("cfg4", n=32, size=64, steps=64, pose="diag", f32=f32, shade=1)
    probe.tf_h = w
    return int((probe.render()[..., 3] > 0).sum())


@pytest.mark.parametrize("f32", [True, False])
def test_lanes_that_pass_the_occupancy_bit_and_are_transparent(R, f32):
    """cfg 4 with the third-axis alpha cleared over the upper half of its range: the (v, g) quad's bit is set, the
    normal work is done, and the product of the two alphas is 0 -- no `hit`, nothing may be blended"""
    sc, ref = _scene("cfg4", 1, f32, "diag", "h_upper_half_clear")
    assert _transparent_behind_the_bit(f32) > 100   # pixels with such a sample (checker: 680 / 693 of 4096)
    a, b = _gather_and_ring(R, sc)
    assert ref[..., 3].max() > 0.05
    assert np.array_equal(a, b)
    assert np.abs(b - ref).max() <= TOL
    if f32:  # (the diagnostic instance -- float voxels, R8k shading -- renders the same frame and counts its turns)
        push_scene(R, sc)
        R.set_option("kernel", 2)
        R.set_option("lockstep", 1 | 16)
        try:
            c = R.render()
            with_maybe, with_hit = R.stat("slab_iters_with_maybe"), R.stat("slab_iters_with_hit")
            lanes_hit = R.stat("slab_hit_lanes")
        finally:
            R.set_option("lockstep", 1)
            R.set_option("kernel", 0)
        assert np.array_equal(c, b)
        assert lanes_hit > 0 and with_maybe >= with_hit > 0, (with_maybe, with_hit)


@pytest.mark.parametrize("f32", [True, False])
def test_rays_that_saturate_right_after_a_reordered_turn(R, f32):
    sc, ref = _scene("cfg3", 1, f32, "diag", "opaque_band")
    a, b = _gather_and_ring(R, sc)
    assert (ref[..., 3] == 1.0).any() and (b[..., 3] == 1.0).any()   # accumulated alpha exactly 1: the ray ended early
    assert np.array_equal(a, b)
    assert np.abs(b - ref).max() <= TOL


def test_first_hit_depth(R):
    sc, _ = _scene("cfg3", 1, True, "diag")
    ref, rd = sc.render(depth=True)
    push_scene(R, sc)
    try:
        R.set_option("kernel", 1)
        ga, gd = R.render(depth=True)
        R.set_option("kernel", 2)
        sa, sd = R.render(depth=True)
        assert R.last_frame_info()[0] == 2
        plain = R.render()
    finally:
        R.set_option("kernel", 0)
    assert np.array_equal(sa, plain) and np.array_equal(sa, ga)
    assert np.array_equal(np.isfinite(gd), np.isfinite(sd))
    fin = np.isfinite(gd)
    assert fin.any() and not fin.all()
    assert np.array_equal(gd[fin], sd[fin])
    assert np.array_equal(fin, np.isfinite(rd)) and np.abs(rd[fin] - sd[fin]).max() <= 1e-4
    assert np.abs(sa - ref).max() <= TOL


@pytest.mark.parametrize("kind,shade,f32", [("cfg3", 1, True), ("cfg3", 2, False), ("cfg4", 1, True)])
def test_big_workgroups_hold_the_normals_in_registers(R, kind, shade, f32):
    """option "tile" 4: 32 x 24 pixels, 12 + 4 waves -- whole voxels read in one batch, ring slots released early"""
    sc, ref = _scene(kind, shade, f32, "diag")
    a, b = _gather_and_ring(R, sc, tile=4)
    assert np.array_equal(a, b)
    assert np.abs(b - ref).max() <= TOL
