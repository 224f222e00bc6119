"""Display-ready frames on the device (include/smk.h "display-ready frames"; simian-spacemonkey_amd/csrc/smk_present.hip):
the conversion kernel against its numpy restatement (tests/_present_ref.py) byte for byte -- fp32 op by op for colour, float64
rounded once for depth: IEEE multiply, add and divide are correctly rounded on both sides, so no tolerance --, rendered frames
through the synchronous entry, two frames in flight through the pipelined pair, a sort-last merge, and the statistics."""
import numpy as np
import pytest

import _present_ref as PR
from _scenes import make_scene, push_scene, tf_cfg2

pytestmark = pytest.mark.gpu
F = np.float32
BG = (0.2, 0.5, 0.9)
CLIP = (1.0, 20.0)   # push_scene's clip planes


def _window(r, w, h):
    """a context that only knows its window: all smk_present_device needs"""
    ident = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    r.set_camera(ident, (-0.1, 0.1, -0.1, 0.1), CLIP, w, h)


def _hand_built_frame(w, h, seed, shift=0):
    """[h][w][4] floats: the quantiser's edge values (every k/255 and its two neighbours among them), rolled by `shift` so that
    they meet every channel, then seeded random values in [-0.25, 1.25]"""
    rng = np.random.default_rng(seed)
    n = w * h * 4
    flat = rng.uniform(-0.25, 1.25, n).astype(F)
    e = np.roll(PR.edge_values(), shift)
    m = min(n, e.size)
    flat[:m] = e[:m]
    return flat.reshape(h, w, 4)


def _hand_built_depth(w, h, seed):
    rng = np.random.default_rng(seed)
    n, f = F(CLIP[0]), F(CLIP[1])
    special = np.array([n, f, np.nextafter(n, F(0)), np.nextafter(n, F(30)), np.nextafter(f, F(0)), np.nextafter(f, F(30)),
                        0.0, -0.0, -1.0, -7.5, np.inf, -np.inf, np.nan, 1e-30, 25.0, 1e30, 1.5, 10.0, 19.999], F)
    d = rng.uniform(0.5, 21.0, w * h).astype(F)
    m = min(d.size, special.size)
    d[:m] = special[:m]
    if d.size > 2 * special.size:
        d[-special.size:] = special[::-1]          # (... and in the last lanes / the tail)
    return d.reshape(h, w)


def _present(r, frame, depth, bg, misalign=0):
    """smk_present_device on host arrays through torch device buffers; misalign: float offset of the outputs (the 4-byte store
    path of buffers that are not 16-byte aligned)"""
    import torch
    h, w = frame.shape[:2]
    d_in = torch.from_numpy(frame).cuda()
    d_out = torch.zeros(h * w + 8, dtype=torch.int32, device="cuda")
    o8 = d_out[misalign:]
    d_dep = d_zw = None
    if depth is not None:
        d_dep = torch.from_numpy(np.concatenate([np.zeros(misalign, F), depth.reshape(-1)])).cuda()
        d_zw = torch.full((h * w + 8,), -5.0, dtype=torch.float32, device="cuda")
    r.present_device(d_in.data_ptr(), o8.data_ptr(), bg=bg,
                     d_depth=d_dep[misalign:].data_ptr() if depth is not None else None,
                     d_zwin=d_zw[misalign:].data_ptr() if depth is not None else None,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert not raw[:misalign].any() and not raw[misalign + h * w:].any(), "wrote outside the frame"
    got8 = raw[misalign:misalign + h * w].view(np.uint8).reshape(h, w, 4)
    gotz = None
    if depth is not None:
        z = d_zw.cpu().numpy()
        assert np.all(z[:misalign] == -5.0) and np.all(z[misalign + h * w:] == -5.0), "wrote outside the depth plane"
        gotz = z[misalign:misalign + h * w].reshape(h, w)
    return got8, gotz


def _same_bytes(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d values differ, first at %s: got %s, want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _same_depth(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32
    _same_bytes(got.view(np.uint32), want.view(np.uint32), what)


# 37 x 29 (1073 pixels: a tail of one, more than one workgroup) and 1 x 1 (tail only) are the tail cases; 64 x 4 has none
@pytest.mark.parametrize("w,h", [(37, 29), (1, 1), (64, 4)])
@pytest.mark.parametrize("bg", [None, BG], ids=["nobg", "bg"])
def test_present_device_equals_the_restatement_on_hand_built_frames(gpu_renderer_factory, w, h, bg):
    r = gpu_renderer_factory()
    try:
        _window(r, w, h)
        shifts = range(0, 785, 49) if w * h == 1 else (0, 1, 2, 3)    # (a 1 x 1 frame holds four values: several frames)
        for k, shift in enumerate(shifts):
            frame = _hand_built_frame(w, h, 11 + k, shift)
            depth = _hand_built_depth(w, h, 31 + k)
            if w * h == 1:
                depth[0, 0] = _hand_built_depth(8, 8, 1).reshape(-1)[k % 19]
            got8, gotz = _present(r, frame, depth, bg)
            _same_bytes(got8, PR.present_rgba8(frame, bg), "rgba8 %dx%d shift %d" % (w, h, shift))
            _same_depth(gotz, PR.window_depth(depth, *CLIP), "window depth %dx%d" % (w, h))
            if bg is not None:
                assert np.all(got8[..., 3] == 255)
        # colour alone (no depth planes), and outputs that are not 16-byte aligned: the 4-byte store path
        frame = _hand_built_frame(w, h, 5, 2)
        depth = _hand_built_depth(w, h, 6)
        got8, _ = _present(r, frame, None, bg)
        _same_bytes(got8, PR.present_rgba8(frame, bg), "rgba8 alone")
        got8, gotz = _present(r, frame, depth, bg, misalign=1)
        _same_bytes(got8, PR.present_rgba8(frame, bg), "rgba8 misaligned")
        _same_depth(gotz, PR.window_depth(depth, *CLIP), "window depth misaligned")
    finally:
        r.close()


def test_present_device_refuses_what_it_cannot_convert(gpu_renderer_factory):
    import torch
    r = gpu_renderer_factory()
    try:
        buf = torch.zeros(64, dtype=torch.float32, device="cuda")
        with pytest.raises(Exception, match="no camera"):
            r.present_device(buf.data_ptr(), buf.data_ptr() + 128)
        _window(r, 2, 2)
        with pytest.raises(Exception, match="together or not at all"):
            r.present_device(buf.data_ptr(), buf.data_ptr() + 128, d_depth=buf.data_ptr())
        with pytest.raises(Exception, match="not in \\[0, 1\\]"):
            r.present_device(buf.data_ptr(), buf.data_ptr() + 128, bg=(0.5, 1.5, 0.0))
        with pytest.raises(Exception, match="16-byte aligned"):
            r.present_device(buf.data_ptr() + 4, buf.data_ptr() + 128)
    finally:
        r.close()


def _scene(kind):
    if kind == "cfg3":
        return make_scene("cfg3", n=32, size=64, steps=64, pose="rot", f32=True, shade=1)
    return make_scene("cfg1", n=32, size=64, steps=64, pose="rot")


def _check_frame(got8, gotz, frame, depth, bg, what):
    _same_bytes(got8, PR.present_rgba8(frame, bg), what + " rgba8")
    if gotz is not None:
        _same_depth(gotz, PR.window_depth(depth, *CLIP), what + " window depth")


@pytest.mark.parametrize("kind,kernel", [("cfg3", 0), ("cfg3", 1), ("cfg3", 2), ("cfg1", 0)])
def test_render_present_equals_the_restatement_of_the_float_frame(gpu_renderer_factory, kind, kernel):
    """both background modes, with and without depth, and a scene depth through the occluded path; option kernel 1 and 2
    where the slice-ring kernel takes the scene"""
    r = gpu_renderer_factory()
    try:
        sc = _scene(kind)
        push_scene(r, sc)
        r.set_option("kernel", kernel)
        frame, depth = r.render(depth=True)
        if kernel:
            assert r.last_frame_info()[0] == kernel
        empty = bool(np.isinf(depth).any())                  # (cfg 1's noise volume covers every pixel of its window)
        assert frame[..., 3].max() > 0.05 and np.isfinite(depth).any() and (empty or kind == "cfg1")
        for bg in (None, BG):
            got8 = r.render_present(bg=bg)
            assert got8.shape == (64, 64, 4) and got8.dtype == np.uint8
            _check_frame(got8, None, frame, depth, bg, "%s kernel %d" % (kind, kernel))
            got8, gotz = r.render_present(bg=bg, depth=True)
            _check_frame(got8, gotz, frame, depth, bg, "%s kernel %d with depth" % (kind, kernel))
            if kernel:
                assert r.last_frame_info()[0] == kernel
        assert got8[..., :3].min() < 255 and (gotz < 1.0).any() and (gotz == 1.0).any() == empty
        # the host's opaque scene in front of half the volume: smk_render_occluded's frame
        zs = np.full((64, 64), np.inf, F)
        zs[:, :32] = float(np.median(depth[np.isfinite(depth)]))
        occ, occ_d = r.render(depth=True, scene_depth=zs)
        assert np.abs(occ - frame).max() > 1e-3 and np.isinf(occ_d).any()    # (here every scene has pixels with no hit)
        got8, gotz = r.render_present(bg=BG, depth=True, scene_depth=zs)
        _check_frame(got8, gotz, occ, occ_d, BG, "occluded")
        zw = PR.window_depth(zs, *CLIP)                       # ... and as window depths, what the host's depth buffer holds
        occ_w, occ_wd = r.render(depth=True, scene_depth=zw, scene_depth_kind=1)
        got8, gotz = r.render_present(depth=True, scene_depth=zw, scene_depth_kind=1)
        _check_frame(got8, gotz, occ_w, occ_wd, None, "occluded by window depths")
        with pytest.raises(Exception, match="bad scene depth kind"):
            r.render_present(scene_depth=zs, scene_depth_kind=7)
    finally:
        r.close()


def test_a_flagged_frame_is_rendered_again_or_fails(gpu_renderer_factory):
    """the synchronous entry's rule for a frame the slice-ring kernel flags (test hook inject_slab_status): auto mode renders it
    again on the gather kernel before anything is returned, a forced kernel fails the call; the pipelined pair the same at end"""
    r = gpu_renderer_factory()
    try:
        sc = _scene("cfg3")
        push_scene(r, sc)
        r.set_option("kernel", 1)
        frame, depth = r.render(depth=True)
        r.set_option("kernel", 2)
        r.set_option("inject_slab_status", 1)
        with pytest.raises(Exception, match="time-out"):
            r.render_present(bg=BG)
        t = r.render_present_begin(bg=BG)
        r.render_present_end(t)                               # (the next forced frame is fine)
        r.set_option("inject_slab_status", 2)
        t = r.render_present_begin(bg=BG)
        with pytest.raises(Exception, match="window outside"):
            r.render_present_end(t)
        with pytest.raises(Exception, match="unknown or has been ended"):
            r.render_present_end(t)                           # (the failed ticket is spent)
        r.set_option("kernel", 0)
        retries = r.stat("slab_retries")
        r.set_option("inject_slab_status", 2)                 # (a new configuration's first trial frame is the slice-ring kernel's)
        got8, gotz = r.render_present(bg=BG, depth=True)
        assert r.stat("slab_retries") == retries + 1 and r.last_frame_info()[0] == 1
        _check_frame(got8, gotz, frame, depth, BG, "rendered again")
    finally:
        r.close()


def test_two_frames_in_flight(gpu_renderer_factory):
    r = gpu_renderer_factory()
    try:
        sa = _scene("cfg3")
        sb = _scene("cfg3")
        sb.tf_vg, sb.tf_h = tf_cfg2()                         # another transfer table
        sb.xform = make_scene("cfg3", n=32, size=64, steps=64, pose="side", f32=True).xform   # ... and another pose
        push_scene(r, sa)
        want_a = r.render_present(bg=BG, depth=True)
        push_scene(r, sb, upload=False)
        want_b = r.render_present(bg=None, depth=True)
        assert (want_a[0] != want_b[0]).mean() > 0.05
        push_scene(r, sa, upload=False)
        ta = r.render_present_begin(bg=BG, depth=True)
        push_scene(r, sb, upload=False)
        tb = r.render_present_begin(bg=None, depth=True)
        assert tb == ta + 1
        # a third frame is refused while both are outstanding, and the window cannot change under them
        with pytest.raises(Exception, match="two frames are in flight already"):
            r.render_present_begin()
        with pytest.raises(Exception, match="window cannot change"):
            r.set_camera(sb.mv(), sb.frustum, CLIP, 48, 48)
        r.set_camera(sb.mv(), sb.frustum, CLIP, 64, 64)      # (the same size is no change)
        a8, az = r.render_present_end(ta)                    # views of slot A's pinned buffers
        _same_bytes(a8, want_a[0], "frame A")
        _same_depth(az, want_a[1], "frame A depth")
        keep8, keepz = a8.copy(), az.copy()
        b8, bz = r.render_present_end(tb)
        _same_bytes(b8, want_b[0], "frame B")
        _same_depth(bz, want_b[1], "frame B depth")
        assert b8.ctypes.data != a8.ctypes.data and bz.ctypes.data != az.ctypes.data
        _same_bytes(a8, keep8, "frame A after B's begin and end")
        _same_depth(az, keepz, "frame A depth after B's end")
        # a ticket ends once; tickets nobody was given are unknown
        for stale in (ta, tb, tb + 1, 0, -3):
            with pytest.raises(Exception, match="unknown or has been ended"):
                r.render_present_end(stale)
        # One more pair.  It is the SECOND begin after A's own, so it takes A's slot (A's pointers, now frame C); B's slot --
        # the other one -- must not be touched by it: B stays valid until the second begin after ITS own.
        keepb8, keepbz = b8.copy(), bz.copy()
        push_scene(r, sa, upload=False)
        tc = r.render_present_begin(bg=BG, depth=True)
        _same_bytes(b8, keepb8, "frame B after C's begin")
        c8, cz = r.render_present_end(tc)
        assert c8.ctypes.data == a8.ctypes.data and cz.ctypes.data == az.ctypes.data
        _same_bytes(c8, want_a[0], "frame C")
        _same_depth(cz, want_a[1], "frame C depth")
        _same_bytes(b8, keepb8, "frame B after C's end")
        _same_depth(bz, keepbz, "frame B depth after C's end")
        # with nothing outstanding the window may change: the slots follow it
        sb.width = sb.height = 40
        push_scene(r, sb, upload=False)
        small = r.render(depth=True)
        got8, gotz = r.render_present(depth=True)
        assert got8.shape == (40, 40, 4)
        _check_frame(got8, gotz, small[0], small[1], None, "after a window change")
    finally:
        r.close()


def test_a_merged_frame_presents_like_any_other(gpu_renderer_factory):
    """two layers merged by smk_composite_over_device, then smk_present_device: the restatement of the merged float frame"""
    import torch
    r = gpu_renderer_factory()
    try:
        w, h = 37, 29
        _window(r, w, h)
        rng = np.random.default_rng(21)
        a = rng.uniform(0.0, 0.7, (2, h * w, 1)).astype(F)
        layers = np.concatenate([rng.uniform(0.0, 1.0, (2, h * w, 3)).astype(F) * a, a], axis=2)   # premultiplied
        d_layers = torch.from_numpy(layers).cuda()
        d_merged = torch.zeros((h * w, 4), dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        r.composite_over_device(d_layers.data_ptr(), 2, [1, 0], h * w, d_merged.data_ptr(), stream=s)
        d_out = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        r.present_device(d_merged.data_ptr(), d_out.data_ptr(), bg=BG, stream=s)
        torch.cuda.synchronize()
        merged = d_merged.cpu().numpy().reshape(h, w, 4)
        over = layers[1] + (1 - layers[1][:, 3:]) * layers[0]
        assert np.abs(merged.reshape(-1, 4) - over).max() <= 1e-6          # (it IS the two-layer over)
        _same_bytes(d_out.cpu().numpy().view(np.uint8).reshape(h, w, 4), PR.present_rgba8(merged, BG), "merged frame")
    finally:
        r.close()


def test_present_statistics(gpu_renderer_factory):
    import torch
    r = gpu_renderer_factory()
    try:
        sc = _scene("cfg1")
        push_scene(r, sc)
        assert r.stat("present_ms") == 0 and r.stat("present_bytes") == 0
        r.render_present()
        assert r.stat("present_ms") > 0 and r.stat("present_bytes") == 64 * 64 * 4
        k, ms, _ = r.last_frame_info()
        assert k in (1, 2) and ms > 0
        r.render_present(depth=True)
        assert r.stat("present_ms") > 0 and r.stat("present_bytes") == 64 * 64 * 8
        t = r.render_present_begin(bg=BG)
        r.render_present_end(t)
        assert r.stat("present_ms") > 0 and r.stat("present_bytes") == 64 * 64 * 4
        # the conversion alone is timed too (the statistic waits for it); it copies nothing to the host
        d_in = torch.zeros((64 * 64, 4), dtype=torch.float32, device="cuda")
        d_out = torch.zeros(64 * 64, dtype=torch.int32, device="cuda")
        r.present_device(d_in.data_ptr(), d_out.data_ptr())
        assert r.stat("present_ms") > 0 and r.stat("present_bytes") == 64 * 64 * 4
    finally:
        r.close()
