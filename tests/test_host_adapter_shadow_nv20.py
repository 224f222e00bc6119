"""gluvv.light.shadow on the GeForce3 platform through the C++ host-side mirror (tests/host/shadow_nv20_main.cpp): the
reference starts NV20VolRen3D2 there (gluvv.cpp:151-159), so the adapter sets its context's shadow_look to 1 and the frame is
the C ABI's NV20-look frame of the same state, bit for bit; on the Radeon 8500 platform it stays the R8k frame."""
import os
import subprocess

import numpy as np
import pytest

from _scenes import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "shadow_nv20_main")
LIGHT, SHADOW, RATE, AMB = (3.0, 4.0, -3.0), (96, 0.5), 2.5, 0.05


def _run(tmp_path, sc, plat, amb=AMB):
    for name, arr in (("vol.u8", sc.data), ("grad.u8", sc.grad), ("deptex.rgba", sc.tf_vg)):
        arr.tofile(tmp_path / name)
    prefix = tmp_path / ("out_" + plat)
    nx, ny, nz = sc.dims
    cmd = [EXE, str(tmp_path / "vol.u8"), str(nx), str(ny), str(nz), str(sc.nelts), str(tmp_path / "grad.u8"),
           str(tmp_path / "deptex.rgba"), str(sc.width), str(sc.height), repr(RATE)] + [repr(float(v)) for v in sc.xform] + \
          [repr(v) for v in LIGHT] + [str(SHADOW[0]), repr(SHADOW[1]), plat, repr(amb), str(prefix)]
    return subprocess.run(cmd, capture_output=True, text=True), prefix


def test_the_driver_builds_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    if torch.cuda.is_available():
        return                                      # (the GPU test below runs it)
    p, _ = _run(tmp_path, make_scene("cfg3", n=16, size=16, shade=2), "nv20")
    assert p.returncode == 3 and "no HIP device" in p.stderr   # loud failure, no CPU path


@pytest.mark.gpu
def test_the_geforce3_platform_draws_the_nv20_look_and_the_radeon_the_r8k_one(tmp_path, gpu_renderer_factory, smk):
    sc = make_scene("cfg3", n=24, size=40, pose="rot", shade=2)
    frames = {}
    for plat in ("nv20", "r8k"):
        p, prefix = _run(tmp_path, sc, plat)
        assert p.returncode == 0, p.stderr
        frames[plat] = np.fromfile(str(prefix) + ".f32", np.float32).reshape(sc.height, sc.width, 4)
        mv = np.fromfile(str(prefix) + ".mv", np.float64)
    r = gpu_renderer_factory()
    try:
        # the adapter's calls (HipVolumeRenderable::init / draw), state for state
        r.upload_volume(sc.data, sc.grad, fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
        r.set_tf2d(sc.tf_vg)                                  # (the raw table: the library corrects it for the rate)
        fr = float(np.float32(0.5) / np.float32(7))           # (the driver's 0.5f / 7)
        r.set_camera(list(mv), (-fr, fr, -fr, fr), (1.0, 20.0), sc.width, sc.height)
        r.set_sampling(RATE, 0, 1.0, 1)
        r.set_shadow(1, *SHADOW)
        r.set_shading("nv20", LIGHT, (0, 0, -7), (0, 0, 0), sc.xform, 0.75, AMB)
        with pytest.raises(smk.SmkError, match="NV20"):
            r.render()                                        # (the C ABI's default look has no NV20 shading)
        r.set_option("shadow_look", 1)
        want = r.render()
        assert want[..., 3].max() > 0.05
        assert np.array_equal(frames["nv20"], want), np.abs(frames["nv20"] - want).max()
        r.set_shadow(0)
        assert np.abs(r.render()[..., :3] - want[..., :3]).max() > 1e-2   # (and it is the shadowed frame)
        r.set_shadow(1, *SHADOW)
        r.set_option("shadow_look", 0)
        r.set_shading("r8k", LIGHT, (0, 0, -7), (0, 0, 0), sc.xform, 0.75, AMB)
        assert np.array_equal(frames["r8k"], r.render())
    finally:
        r.close()
