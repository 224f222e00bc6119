"""Display-ready frames through the C++ host-side mirror (HipVolumeRenderable::present / framebuffer8 / depthbuffer), driven by
tests/host/present_main.cpp the way Simian's display() drives a renderer: two poses drawn in the default float mode, in the
pipelined present mode and in the synchronous one.  The bytes the host would blit must be the present rule
(tests/_present_ref.py) applied to the float frames of the same run."""
import os
import subprocess

import numpy as np
import pytest

import _present_ref as PR
from _scenes import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "present_main")
WHITE = (1.0, 1.0, 1.0)


def _run(tmp_path, sc, shade, rate, deptex, pose_b, bgcolor):
    vol = tmp_path / "vol.u8"
    sc.data.tofile(vol)
    grad = "-"
    if sc.grad is not None:
        grad = tmp_path / "grad.u8"
        sc.grad.tofile(grad)
    dep = "-"
    if deptex is not None:
        dep = tmp_path / "deptex.rgba"
        deptex.tofile(dep)
    prefix = tmp_path / "out"
    nx, ny, nz = sc.dims
    cmd = [EXE, str(vol), str(nx), str(ny), str(nz), str(sc.nelts), str(grad), str(dep), str(sc.width), str(sc.height),
           repr(rate), str(shade)] + [repr(float(v)) for v in sc.xform] + [repr(float(v)) for v in pose_b] + [str(bgcolor), str(prefix)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    h, w = sc.height, sc.width

    def load(suffix):
        if suffix.endswith("f32"):
            return np.fromfile(str(prefix) + suffix, np.float32).reshape(h, w, 4)
        if suffix.endswith("zwin"):
            return np.fromfile(str(prefix) + suffix, np.float32).reshape(h, w)
        return np.fromfile(str(prefix) + suffix, np.uint8).reshape(h, w, 4)
    return p, load


def test_present_driver_builds_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    if torch.cuda.is_available():
        return                                      # (the GPU tests below run it)
    sc = make_scene("cfg1", n=16, size=16)
    p, _ = _run(tmp_path, sc, 1, 1.0, None, sc.xform, 1)
    assert p.returncode == 3 and "no HIP device" in p.stderr   # loud failure, no CPU path


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bgcolor", [("cfg3", 0), ("cfg3", 1), ("cfg1", 0)])
def test_framebuffer8_is_the_present_rule_of_the_float_frames(tmp_path, O, kind, bgcolor):
    if kind == "cfg3":
        sc = make_scene("cfg3", n=24, size=40, pose="rot", shade=1)
        shade, rate, deptex = 3, 2.5, sc.tf_vg
    else:
        sc = make_scene("cfg1", n=24, size=40, pose="rot")
        shade, rate, deptex = 1, 1.5, None
    pose_b = O.rotation((.2, 1, .1), 75)
    p, load = _run(tmp_path, sc, shade, rate, deptex, pose_b, bgcolor)
    assert p.returncode == 0, p.stderr
    fa, fb = load(".a.f32"), load(".b.f32")
    assert fa[..., 3].max() > 0.05 and np.abs(fa - fb).max() > 0.05          # two different frames, something in them
    bg = WHITE if bgcolor == 0 else None                                      # gluvv.env.bgColor == 0: white (gluvv.cpp:607)
    want_a, want_b = PR.present_rgba8(fa, bg), PR.present_rgba8(fb, bg)
    assert (want_a != want_b).mean() > 0.01
    # pipelined: the first draw() has nothing to hand over, the second hands over the FIRST frame, flush() the second
    assert not load(".p1.rgba8").any()
    assert np.array_equal(load(".p2.rgba8"), want_a)
    assert np.array_equal(load(".p3.rgba8"), want_b)
    # synchronous: one draw() one frame
    assert np.array_equal(load(".s1.rgba8"), want_a)
    assert np.array_equal(load(".s2.rgba8"), want_b)
    empty = fa[..., 3] == 0
    assert empty.any() or kind == "cfg1"                                      # (cfg 1's noise volume covers its whole window)
    if bgcolor == 0:
        assert np.all(want_a[..., 3] == 255) and np.all(want_a[empty] == 255)                    # white where the volume is not
    else:
        assert not want_a[empty].any()
    # the depth buffers: the cleared value where the frame is empty, inside (0, 1) on the volume; both modes the same frame
    za, zb = load(".p2.zwin"), load(".p3.zwin")
    assert np.array_equal(zb, load(".s2.zwin")) and not np.array_equal(za, zb)
    assert np.all(za[empty] == 1.0)
    hit = fa[..., 3] > 0.01
    assert hit.any() and np.all((za[hit] > 0.0) & (za[hit] < 1.0))
