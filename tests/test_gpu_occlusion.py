"""Frames occluded by the host's opaque scene depth (smk.h smk_render_occluded[_device]; the reference's depth test, GL_LESS
with depth writes off): a sample exists only where its view depth -- the value depth_out reports -- is less than the pixel's
scene depth.  Neutral buffers change no bit; fronto-parallel and tilted occluders give the CPU checker's frame with the
equivalent free clip plane; the gather and slice-ring kernels stay bit-identical on arbitrary depth fields; with shadows
only the eye pass is occluded; what cannot be done is refused with the reason."""
import zlib

import numpy as np
import pytest

from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu
TOL = 1e-4
INF = np.float32(np.inf)
VIEW, WINDOW = 0, 1
ZFAR = 20.0   # push_scene's far plane


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


def _plane_depths(R, sc):
    """float64 view depth of every plane of the view-aligned frame: (tau0 + m dtau) znear"""
    rc = R.raycoef()
    return (rc.tau0 + np.arange(rc.nplanes, dtype=np.float64) * rc.dtau) * sc.znear, rc


def _window_depth(d, n, f):
    """what glReadPixels(GL_DEPTH_COMPONENT, GL_FLOAT) returns for view depth d (computed in float64)"""
    return ((f - f * n / np.asarray(d, np.float64)) / (f - n)).astype(np.float32)


def _depth_rule(rd, gd):
    """the parity tests' depth rule: +inf at the same pixels, the finite depths within 1e-4"""
    fin = np.isfinite(rd)
    assert np.array_equal(fin, np.isfinite(gd))
    if fin.any():
        assert np.abs(rd[fin] - gd[fin]).max() <= 1e-4


def _set(R, kernel=None, blend=None):
    if kernel is not None:
        R.set_option("kernel", kernel)
    if blend is not None:
        R.set_blend(blend)


@pytest.fixture(autouse=True)
def _restore(R):
    yield
    R.set_option("kernel", 0)
    R.set_blend(0)
    R.set_option("shadow_march", 1)
    R.set_option("shadow_fused", 0)


# ------------------------------------------------------------------------------------------------ 1. neutral buffers

@pytest.mark.parametrize("shadows", [False, True])
@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("kernel", [0, 1, 2])
def test_neutral_buffers_change_no_bit(R, kernel, blend, shadows):
    """+inf view depths, window depths of 1 (a cleared buffer) and NaN in either kind: RGBA and depth bit-identical to
    render() on the same ray-marcher, through the host and the device entry.  (Auto mode may take either; the two agree
    bit for bit except on back-to-front frames, which the slice-ring kernel composites front to back: smk.h smk_set_blend.)"""
    import torch
    sc = make_scene("cfg3", size=48, steps=48, f32=True, shade=1)
    if shadows:
        sc.light_pos = (3, 4, -3)
        sc.shadow = (64, 0.7)
    push_scene(R, sc)
    h, w = sc.height, sc.width
    plain = {}
    for k in (1, 2):
        _set(R, k, blend)
        plain[k] = R.render(depth=True)
        assert R.last_frame_info()[0] == k
    _set(R, kernel, blend)
    ref, rd = plain[kernel or 2]
    assert ref[..., 3].max() > 0.05 and np.isfinite(rd).mean() > 0.1, "vacuous scene"
    buffers = [(np.full((h, w), INF), VIEW), (np.ones((h, w), np.float32), WINDOW),
               (np.full((h, w), np.nan, np.float32), VIEW), (np.full((h, w), np.nan, np.float32), WINDOW)]
    for zs, kind in buffers:
        for _ in range(2 if kernel == 0 else 1):   # (auto mode: trial frames of both ray-marchers)
            got, gd = R.render(depth=True, scene_depth=zs, scene_depth_kind=kind)
            used = R.last_frame_info()[0]
            assert used == kernel or (kernel == 0 and used in (1, 2)), used
            assert np.array_equal(got, plain[used][0]) and np.array_equal(gd, plain[used][1]), (kind, used)
        # the device entry, the same bits
        dzs = torch.from_numpy(zs).cuda()
        drgba = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
        ddep = torch.zeros((h * w,), dtype=torch.float32, device="cuda")
        R.render_device(drgba.data_ptr(), ddep.data_ptr(), None, d_scene_depth=dzs.data_ptr(), scene_depth_kind=kind)
        torch.cuda.synchronize()
        used = R.last_frame_info()[0]
        assert np.array_equal(drgba.cpu().numpy().reshape(h, w, 4), plain[used][0])
        assert np.array_equal(ddep.cpu().numpy().reshape(h, w), plain[used][1])


def test_null_buffer_is_the_plain_frame(R):
    sc = make_scene("cfg3", f32=True, shade=1)
    push_scene(R, sc)
    ref, rd = R.render(depth=True)
    got, gd = R.render(depth=True, scene_depth=None)
    assert np.array_equal(got, ref) and np.array_equal(gd, rd)


# ------------------------------------------------------------------------------ 2. fronto-parallel occluders vs checker

def _blocky_levels(R, sc, rng):
    """a piecewise-constant scene depth (8x8 pixel blocks) at levels midway between two plane depths -- in front of the
    volume, inside it and behind it -- and the level index of every pixel"""
    pd, rc = _plane_depths(R, sc)
    n = rc.nplanes
    planes = [-3, n // 5, (2 * n) // 5, n // 2, (3 * n) // 5, (4 * n) // 5, n + 3]
    levels = np.array([(rc.tau0 + (m + 0.5) * rc.dtau) * sc.znear for m in planes], np.float64)
    assert levels.min() > 0
    h, w = sc.height, sc.width
    blocks = rng.integers(0, len(levels), ((h + 7) // 8, (w + 7) // 8))
    idx = np.kron(blocks, np.ones((8, 8), np.int64))[:h, :w]
    return levels, idx


def _checker_occluded(sc, levels, idx, blend):
    """the checker's frame with the free clip plane (0, 0, 1, d) that keeps the near side, pixel by pixel per level"""
    h, w = sc.height, sc.width
    ref = np.zeros((h, w, 4), np.float32)
    rd = np.full((h, w), np.inf, np.float32)
    for k, d in enumerate(levels):
        sel = idx == k
        if not sel.any():
            continue
        sc.clip_plane = (0.0, 0.0, 1.0, float(d))
        f, fd = sc.render(blend=blend, depth=True)
        ref[sel], rd[sel] = f[sel], fd[sel]
    sc.clip_plane = None
    return ref, rd


# (kernel, kind, f32, shade, perturbation): both ray-marchers on u8 and f32 volumes, 2-D and 3-D tables; perturbation on
# the gather kernel (the slice-ring kernel does not take it)
FRONTO = [(k, "cfg3", False, 1, False) for k in (1, 2)] + [(k, "cfg3", True, 1, False) for k in (1, 2)] + \
         [(k, "cfg2", True, 0, False) for k in (1, 2)] + [(k, "tf3d", False, 1, False) for k in (1, 2)] + \
         [(1, "cfg3", False, 1, True)]


@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("kernel,kind,f32,shade,pert", FRONTO, ids=["-".join(str(x) for x in c) for c in FRONTO])
def test_fronto_parallel_occluders_match_the_checker(R, kernel, kind, f32, shade, pert, blend):
    sc = make_scene(kind, size=64, steps=48, f32=f32, shade=shade, pert=pert)
    push_scene(R, sc)
    _set(R, kernel, blend)
    levels, idx = _blocky_levels(R, sc, np.random.default_rng(zlib.crc32(repr((kind, f32, blend)).encode())))
    ref, rd = _checker_occluded(sc, levels, idx, blend)
    assert ref[..., 3].max() > 0.05 and np.isfinite(rd).mean() > 0.05, "vacuous scene"
    got, gd = R.render(depth=True, scene_depth=levels[idx].astype(np.float32), scene_depth_kind=VIEW)
    assert R.last_frame_info()[0] == kernel
    assert np.abs(got - ref).max() <= TOL, f"max abs err {np.abs(got - ref).max()}"
    _depth_rule(rd, gd)
    # the occluder does something: the frame is not the plain one
    assert not np.array_equal(got, R.render())


# -------------------------------------------------------------------------------- 3. tilted plane in window depths

@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("f32", [False, True])
def test_tilted_plane_in_window_depths(R, kernel, f32):
    sc = make_scene("cfg3", size=64, steps=64, f32=f32, shade=1)
    push_scene(R, sc)
    _set(R, kernel, 0)
    pd, rc = _plane_depths(R, sc)
    zn = sc.znear
    d0 = float(pd[len(pd) // 2] + 0.3 * rc.dtau * zn)
    sx, sy = 0.15, -0.1                       # eye-space plane sx x + sy y + z + d0 = 0; kept: >= 0 (the near side)
    px = (np.arange(sc.width, dtype=np.float64) + 0.5) * rc.pxs + rc.pxl
    py = (np.arange(sc.height, dtype=np.float64) + 0.5) * rc.pys + rc.pyl
    # along a pixel's ray the point at view depth d is (px d / zn, py d / zn, -d): it meets the plane at D
    D = d0 / (1.0 - (sx * px[None, :] + sy * py[:, None]) / zn)
    assert (D > 0).all()
    zw = _window_depth(D, zn, ZFAR)
    sc.clip_plane = (sx, sy, 1.0, d0)
    ref, rd = sc.render(depth=True)
    sc.clip_plane = None
    got, gd = R.render(depth=True, scene_depth=zw, scene_depth_kind=WINDOW)
    assert R.last_frame_info()[0] == kernel
    # pixels with a sample within 1e-4 (relative) of the plane are left out: float32 window depths cannot place it
    near = (np.abs(pd[None, None, :] - D[..., None]) / D[..., None] <= 1e-4).any(-1)
    keep = ~near
    assert keep.mean() >= 0.9, keep.mean()
    assert ref[keep][..., 3].max() > 0.05
    err = np.abs(got - ref)[keep].max()
    assert err <= TOL, f"max abs err {err}"
    _depth_rule(rd[keep], gd[keep])
    assert np.isfinite(gd).mean() > 0.05 and not np.array_equal(got, R.render())


# ----------------------------------------------------------------------------------- 4. an arbitrary depth field

def _sphere_field(R, sc, seed=7):
    pd, rc = _plane_depths(R, sc)
    h, w = sc.height, sc.width
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    r2 = ((x - 0.45 * w) ** 2 + (y - 0.55 * h) ** 2) / (0.35 * min(w, h)) ** 2
    mid = pd[len(pd) // 2]
    depth = np.where(r2 < 1, mid - 0.6 * (pd[-1] - pd[0]) * np.sqrt(np.clip(1 - r2, 0, 1)), pd[-1] + 1.0)
    depth += np.random.default_rng(seed).normal(0, 0.05 * (pd[-1] - pd[0]), depth.shape)
    return depth.astype(np.float32)


@pytest.mark.parametrize("blend", [0, 1, 2])
@pytest.mark.parametrize("kind,f32,shade", [("cfg3", False, 1), ("cfg3", True, 2), ("tf3d", True, 0)])
def test_depth_field_gather_equals_slice_ring(R, kind, f32, shade, blend):
    sc = make_scene(kind, size=72, steps=64, f32=f32, shade=shade, pose="side")
    push_scene(R, sc)
    zs = _sphere_field(R, sc)
    out = {}
    for kern in (1, 2):
        _set(R, kern, blend)
        out[kern] = R.render(depth=True, scene_depth=zs)
        assert R.last_frame_info()[0] == kern
    assert out[1][0][..., 3].max() > 0.05
    if blend == 1:   # (back to front: the slice-ring kernel composites the same samples front to back, smk_set_blend)
        assert np.abs(out[1][0] - out[2][0]).max() <= 2e-5, "gather vs slice-ring RGBA"
    else:
        assert np.array_equal(out[1][0], out[2][0]), "gather vs slice-ring RGBA"
    assert np.array_equal(out[1][1], out[2][1]), "gather vs slice-ring depth"
    # every composited sample lies in front of the scene
    fin = np.isfinite(out[1][1])
    assert fin.mean() > 0.05 and (out[1][1][fin] < zs[fin]).all()


@pytest.mark.parametrize("kernel", [1, 2])
def test_raising_the_scene_depth_never_lowers_alpha(R, kernel):
    sc = make_scene("cfg3", size=64, steps=64, f32=True, shade=1)
    push_scene(R, sc)
    _set(R, kernel, 0)
    pd, _ = _plane_depths(R, sc)
    zs = _sphere_field(R, sc, seed=11)
    prev = R.render(scene_depth=zs)[..., 3]
    grew = False
    for step in (0.05, 0.1, 0.2, 0.4, 1.0):
        cur = R.render(scene_depth=(zs + step * (pd[-1] - pd[0])).astype(np.float32))[..., 3]
        assert (cur >= prev).all(), f"alpha fell where the scene depth rose (step {step})"
        grew |= bool((cur > prev).any())
        prev = cur
    assert grew


# ------------------------------------------------------------------------------------------------------- 5. shadows

@pytest.mark.parametrize("kind,f32,shade,light", [("cfg3", True, 1, (3, 4, -3)), ("cfg3", False, 0, (-2, 3, 4)),
                                                  ("tf3d", False, 1, (5, 1, 0.5))])
def test_shadows_occlude_the_eye_pass_only(R, kind, f32, shade, light):
    sc = make_scene(kind, size=64, steps=64, f32=f32, shade=shade)
    sc.light_pos = light
    sc.shadow = (64, 0.75)
    push_scene(R, sc)
    pd, _ = _plane_depths(R, sc)      # (the view-aligned planes span the volume's view depths)
    h, w = sc.height, sc.width
    # the left half in front of the volume, the right half behind it
    zs = np.full((h, w), 2.0 * pd[-1] + 10.0, np.float32)
    zs[:, : w // 2] = 0.5 * pd[0]
    assert 0 < 0.5 * pd[0]
    plain, pdep = R.render(depth=True)
    plainL = R.light_buffer()
    out = {}
    for form in ("gather", "slab", "per_slice", "fused"):
        R.set_option("kernel", {"gather": 1, "slab": 2}.get(form, 0))
        R.set_option("shadow_march", 0 if form == "per_slice" else 1)
        R.set_option("shadow_fused", 1 if form == "fused" else 0)
        out[form] = R.render(depth=True, scene_depth=zs)
        assert R.last_frame_info()[0] == {"gather": 1, "slab": 2}.get(form, 3), form
        assert np.array_equal(R.light_buffer(), plainL), f"{form}: the light buffer changed"
    g, gd = out["gather"]
    assert np.array_equal(g, out["slab"][0]) and np.array_equal(gd, out["slab"][1]), "gather vs slice-ring"
    assert np.array_equal(out["per_slice"][0], out["fused"][0]), "per-slice vs fused RGBA"
    for form in ("slab", "per_slice", "fused"):
        assert np.array_equal(gd, out[form][1]), f"{form}: depth"
    assert np.abs(out["per_slice"][0] - g).max() <= TOL
    # in front: nothing; behind: the unoccluded frame (and the checker's)
    assert not g[:, : w // 2].any() and np.isinf(gd[:, : w // 2]).all()
    assert np.array_equal(g[:, w // 2:], plain[:, w // 2:]) and np.array_equal(gd[:, w // 2:], pdep[:, w // 2:])
    ref, _ = sc.render_shadow()
    assert ref[:, w // 2:, 3].max() > 0.05
    assert np.abs(g[:, w // 2:] - ref[:, w // 2:]).max() <= TOL


# -------------------------------------------------------------------------------------------------------- 7. errors

def test_bad_kind_and_column_stream_are_refused(R, smk):
    sc = make_scene("cfg3", f32=True)
    push_scene(R, sc)
    zs = np.full((sc.height, sc.width), INF)
    with pytest.raises(smk.SmkError, match="scene depth kind"):
        R.render(scene_depth=zs, scene_depth_kind=2)
    with pytest.raises(smk.SmkError, match="scene depth kind"):
        R.render(scene_depth=zs, scene_depth_kind=-1)
    with pytest.raises(ValueError):
        R.render(scene_depth=zs[1:])
    R.set_option("kernel", 3)
    with pytest.raises(smk.SmkError, match=r"not applicable: scene depth$"):
        R.render(scene_depth=zs)
    R.set_option("kernel", 0)
    R.render(scene_depth=zs)          # (the context renders on)
    assert R.last_frame_info()[0] in (1, 2)


def test_frame_info_counts_the_scene_depth(R):
    sc = make_scene("cfg3", f32=True)
    push_scene(R, sc)
    R.render()
    plain = R.last_frame_info()[2]
    R.render(scene_depth=np.full((sc.height, sc.width), INF))
    assert R.last_frame_info()[2] == plain + 4.0 * sc.width * sc.height
