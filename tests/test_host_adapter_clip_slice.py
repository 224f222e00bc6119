"""HipVolumeRenderable::draw with the clip-plane widget's state in gluvv.clip (tests/host/clip_slice_main.cpp): on, ortho,
oaxis, vpos cut the volume as before, and corners, alpha, pos, dir now draw the widget's data slice -- the same frame as
the binding called directly with the dv the reference computes from eye, pos and dir."""
import os
import subprocess

import numpy as np
import pytest

from _clip_slice_cases import clip_vpos, widget_corners
from _scenes import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "clip_slice_main")
RATE = 2.5
ALPHA = 0.55


def _csv(v):
    return ",".join(repr(float(x)) for x in np.asarray(v).reshape(-1))


def _run(tmp_path, sc, extra):
    vol, grad, dep, out = (tmp_path / n for n in ("vol.u8", "grad.u8", "deptex.rgba", "frame.f32"))
    sc.data.tofile(vol)
    sc.grad.tofile(grad)
    sc.tf_vg.tofile(dep)
    nx, ny, nz = sc.dims
    cmd = [EXE, str(vol), str(nx), str(ny), str(nz), str(sc.nelts), str(grad), str(dep), str(sc.width), str(sc.height),
           repr(RATE), "3"] + [repr(float(v)) for v in sc.xform] + [str(out)] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True), out


def test_driver_is_built():
    assert os.path.exists(EXE), "build with __graft_entry__.build()"


@pytest.mark.gpu
@pytest.mark.parametrize("plat,look,shade", [(0, "r8k", "r8k"), (5, "nv20", "nv20")])
@pytest.mark.parametrize("cdir", [(1.0, 0.2, -0.6), (-1.0, 0.1, 0.7)])
def test_draw_passes_the_widget_state(tmp_path, gpu_renderer_factory, plat, look, shade, cdir):
    oaxis = 1
    sc = make_scene("cfg3", n=24, size=40, pose="rot", shade=1)
    vpos = clip_vpos(oaxis, sc.fsize)
    corners = widget_corners(oaxis, vpos, sc.fsize)
    pos = (0.3, -0.1, 0.2)
    # dv as renderVolume computes it (R8kVolRen3D.cpp:273-281), in float
    vd = np.array(sc.eye, np.float32) - np.array(pos, np.float32)
    cd = np.array(cdir, np.float32)
    dv = float(np.dot(vd / np.linalg.norm(vd), cd / np.linalg.norm(cd)))
    assert abs(dv) > 0.1
    R = gpu_renderer_factory()
    try:
        R.upload_volume(sc.data, sc.grad, fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
        R.set_tf2d(sc.tf_vg)
        R.set_clip(oaxis, vpos)
        R.set_camera(sc.mv(), sc.frustum, (1.0, 20.0), sc.width, sc.height)
        R.set_sampling(RATE, 0, 1.0, 1)
        R.set_shading(shade, sc.light_pos, sc.eye, sc.at, sc.xform, 0.75, 0.05)
        plain = R.render()
        R.set_clip_slice(corners, ALPHA, dv, look)
        want = R.render()
        want_pass = R.stat("clip_slice_pass")
    finally:
        R.close()
    assert want_pass == (1 if dv < 0 else 2)
    assert plain[..., 3].max() > 0.05 and (np.abs(want - plain).max(axis=-1) > 1e-3).sum() > 100, "vacuous"
    args = ["on=1", "ortho=1", "oaxis=%d" % oaxis, "alpha=%r" % ALPHA, "vpos=" + _csv(vpos), "pos=" + _csv(pos),
            "dir=" + _csv(cdir), "corners=" + _csv(corners), "plat=%d" % plat]
    p, out = _run(tmp_path, sc, args)
    assert p.returncode == 0, p.stderr
    got = np.fromfile(out, np.float32).reshape(sc.height, sc.width, 4)
    assert np.abs(got - want).max() <= 2e-5, np.abs(got - want).max()   # (auto mode may take either ray-marcher)
    # the widget switched off: the plain, uncut frame -- no slice without the plane
    p, out = _run(tmp_path, sc, ["on=0"] + args[1:])
    assert p.returncode == 0, p.stderr
    off = np.fromfile(out, np.float32).reshape(sc.height, sc.width, 4)
    assert np.abs(off - want).max() > 1e-2
