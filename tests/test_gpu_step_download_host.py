"""The shown step read back and saved through the host-side mirror (tests/host/step_download_main.cpp):
HipVolumeRenderer::downloadStep and HipVolumeRenderable::saveTimeStep over a three-step series at setTimeFraction(0.5).  What
the adapter hands over, and what its files hold when they are read back with VolumeFiles' own readers (tests/host/files_main:
smkfiles::load_trex, read_nrrd), is the binding's download of the same blend, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import _step_read_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "step_download_main")
FILES = os.path.join(ROOT, "tests", "host", "files_main")
DIMS = (21, 13, 7)
GDM = {1: 0, 3: 9}                                          # gluvvDataMode: V1, VGH
T, FRAC = 1, 0.5


def _series(dtype, nelts):
    return [D.volume(dtype, nelts, DIMS, seed)[0] for seed in (1, 2, 3)]


def _drive(tmp_path, dtype, nelts):
    steps = _series(dtype, nelts)
    paths = []
    for i, s in enumerate(steps):
        p = tmp_path / ("step%d.raw" % i)
        s.tofile(p)
        paths.append(str(p))
    out = tmp_path / "got"
    cmd = [EXE] + [str(n) for n in DIMS] + [str(nelts), str(int(dtype == "u16")), str(GDM[nelts]), str(T), repr(FRAC), str(out)] + paths
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout, p.stderr)
    return steps, out, p


def _binding_blend(factory, steps, nelts):
    """the binding's download of the same blend: (data, grad)"""
    R = factory()
    try:
        R.set_timestep_cache(4)
        R.upload_volume(steps[0], None, dmode=D.DMODE[nelts])
        R.upload_timestep(1, steps[1], None, dmode=D.DMODE[nelts])
        R.upload_timestep(2, steps[2], None, dmode=D.DMODE[nelts])
        R.blend_timesteps(T, T + 1, FRAC, 9)
        return R.download_timestep(9)
    finally:
        R.close()


def _downloaded(out, dtype, nelts):
    nx, ny, nz = DIMS
    box = np.fromfile(str(out) + ".box", np.int32)
    assert list(box) == [0, 0, 0, nx, ny, nz]
    data = np.fromfile(str(out) + ".data", D.NP[dtype]).reshape(nz, ny, nx, nelts)
    grad = np.fromfile(str(out) + ".grad", np.uint8).reshape(nz, ny, nx, 3)
    return data, grad


def test_driver_is_built():
    assert os.path.exists(EXE), "build with __graft_entry__.build()"


@pytest.mark.gpu
@pytest.mark.parametrize("nelts", [1, 3])
def test_the_shown_blend_is_downloaded_and_saved(gpu_renderer_factory, tmp_path, nelts):
    steps, out, p = _drive(tmp_path, "u8", nelts)
    assert "downloadStep 1" in p.stdout and "saveTimeStep 1" in p.stdout, (p.stdout, p.stderr)
    want, wgrad = _binding_blend(gpu_renderer_factory, steps, nelts)
    assert not any(np.array_equal(want, s) for s in steps), "vacuous: the blend is one of the steps"
    data, grad = _downloaded(out, "u8", nelts)
    assert np.array_equal(data, want) and np.array_equal(grad, wgrad) and (grad == 128).all()
    back = tmp_path / "back.u8"
    if nelts == 1:                                          # writeAll's .trex and its one raw brick, through load_trex
        assert os.path.exists(str(out) + ".saved.trex") and os.path.exists(str(out) + ".saved.0000.00")
        q = subprocess.run([FILES, "load", str(out) + ".saved.trex", "0", str(back)], capture_output=True, text=True)
        assert q.returncode == 0, q.stderr
        assert "bricks=1" in q.stdout and "isize=%d %d %d" % DIMS in q.stdout
    else:                                                   # genVGH's writer, through read_nrrd
        assert os.path.exists(str(out) + ".saved.nrrd") and not os.path.exists(str(out) + ".saved.trex")
        q = subprocess.run([FILES, "nrrd-read", str(out) + ".saved.nrrd", str(back)], capture_output=True, text=True)
        assert q.returncode == 0, q.stderr
    assert np.array_equal(np.fromfile(back, np.uint8), want.ravel())


@pytest.mark.gpu
def test_a_u16_series_is_served_by_download_and_refused_by_save(gpu_renderer_factory, tmp_path):
    steps, out, p = _drive(tmp_path, "u16", 1)
    assert "downloadStep 1" in p.stdout and "saveTimeStep 0" in p.stdout, (p.stdout, p.stderr)
    assert "no 16-bit / float writer" in p.stderr
    assert not os.path.exists(str(out) + ".saved.trex") and not os.path.exists(str(out) + ".saved.nrrd")
    want, wgrad = _binding_blend(gpu_renderer_factory, steps, 1)
    data, grad = _downloaded(out, "u16", 1)
    assert data.dtype == np.uint16 and np.array_equal(data, want) and np.array_equal(grad, wgrad)
