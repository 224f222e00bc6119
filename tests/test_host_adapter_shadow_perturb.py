"""gluvv.pert.on and gluvv.light.shadow together through the C++ host-side mirror (tests/host/shadow_perturb_main.cpp): the
adapter opts its context into perturbed frames with shadows (option shadow_perturb), as the perturbing renderer it mirrors
draws them, and its frame is the C ABI's own, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from _scenes import make_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "shadow_perturb_main")
LIGHT, SHADOW, PERT, RATE = (3.0, 4.0, -3.0), (96, 0.5), (0.2, 0.1, 0.2, 2.1), 2.5


def _run(tmp_path, sc):
    for name, arr in (("vol.u8", sc.data), ("grad.u8", sc.grad), ("deptex.rgba", sc.tf_vg)):
        arr.tofile(tmp_path / name)
    prefix = tmp_path / "out"
    nx, ny, nz = sc.dims
    cmd = [EXE, str(tmp_path / "vol.u8"), str(nx), str(ny), str(nz), str(sc.nelts), str(tmp_path / "grad.u8"),
           str(tmp_path / "deptex.rgba"), str(sc.width), str(sc.height), repr(RATE)] + [repr(float(v)) for v in sc.xform] + \
          [repr(v) for v in LIGHT] + [str(SHADOW[0]), repr(SHADOW[1])] + [repr(v) for v in PERT] + [str(prefix)]
    return subprocess.run(cmd, capture_output=True, text=True), prefix


def test_the_driver_builds_and_refuses_to_run_without_a_gpu(tmp_path):
    import torch
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    if torch.cuda.is_available():
        return                                      # (the GPU test below runs it)
    p, _ = _run(tmp_path, make_scene("cfg3", n=16, size=16, shade=1))
    assert p.returncode == 3 and "no HIP device" in p.stderr   # loud failure, no CPU path


@pytest.mark.gpu
def test_both_switches_on_draw_the_frame_of_the_binding_with_the_option_on(tmp_path, gpu_renderer_factory, smk):
    sc = make_scene("cfg3", n=24, size=40, pose="rot", shade=1)
    p, prefix = _run(tmp_path, sc)
    assert p.returncode == 0, p.stderr
    got = np.fromfile(str(prefix) + ".f32", np.float32).reshape(sc.height, sc.width, 4)
    mv = np.fromfile(str(prefix) + ".mv", np.float64)
    noise = np.fromfile(str(prefix) + ".noise", np.uint8).reshape(32, 32, 32, 4)
    r = gpu_renderer_factory()
    try:
        # the adapter's calls (HipVolumeRenderable::init / draw), state for state
        r.upload_volume(sc.data, sc.grad, fsize=tuple(float(f) for f in sc.fsize), dmode="VGH")
        r.set_tf2d(sc.tf_vg)                                  # (the raw table: the library corrects it for the rate)
        fr = float(np.float32(0.5) / np.float32(7))           # (the driver's 0.5f / 7)
        r.set_camera(list(mv), (-fr, fr, -fr, fr), (1.0, 20.0), sc.width, sc.height)
        r.set_sampling(RATE, 0, 1.0, 1)
        r.set_shading("r8k", LIGHT, (0, 0, -7), (0, 0, 0), sc.xform, 0.75, 0.05)
        r.set_perturb(noise, PERT[:2] + (0, 0), PERT[2:] + (4.5, 8.7))
        r.set_shadow(1, *SHADOW)
        with pytest.raises(smk.SmkError, match="perturbation"):
            r.render()                                        # (the C ABI's default: refused)
        r.set_option("shadow_perturb", 1)
        want = r.render()
        assert r.last_frame_info()[0] == 1
        assert want[..., 3].max() > 0.05
        assert np.array_equal(got, want), np.abs(got - want).max()
        r.set_perturb(None, None, None)
        assert np.abs(r.render() - want).max() > 1e-2         # (and it is the perturbed frame)
    finally:
        r.close()
