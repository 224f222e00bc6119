"""A 16-bit data set from disk through the host-side mirror (tests/host/u16_adapter_main.cpp): VolumeFiles' 16-bit load,
HipVolumeRenderable::useU16, init() / draw() -- against the CPU checker on the decoded voxels, and against the same data
set taken the reference's 8-bit way."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _u16_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "u16_adapter_main")
RATE = 1.5


def _dataset(tmp_path):
    """the fine-structure volume's value channel as a big-endian ushort file; two voxels span the whole range, so that
    the loader's min/max map is the identity"""
    native = np.array(U.fine_volume()[..., 0])
    native[0, 0, 0], native[-1, -1, -1] = 0, 65535
    nz, ny, nx = native.shape
    raw = tmp_path / "ct"
    native.astype(">u2").tofile(raw)
    m = float(max(nx, ny, nz))
    trex = tmp_path / "ct.trex"
    trex.write_text("Data Set Name: ct\nData Set Files: %s\nNumber of Time Steps: 1, 0, 0\nDon't append numbers\n"
                    "Data Type: ushort\nEndian: big\nVolume Size int: %d, %d, %d\nVolume Size float: %.9g, %.9g, %.9g\n"
                    "Number of Sub Volumes: 1\nSubVolume {\n Size int: %d, %d, %d\n Size float: %.9g, %.9g, %.9g\n"
                    " Pos int: 0, 0, 0\n Pos float: 0, 0, 0\n}\n"
                    % (raw, nx, ny, nz, nx / m, ny / m, nz / m, nx, ny, nz, nx / m, ny / m, nz / m))
    return native, trex


def _run(tmp_path, trex, u16, sc, name):
    dep = tmp_path / "deptex.rgba"
    U.fine_table().tofile(dep)
    out = tmp_path / name
    cmd = [EXE, str(trex), str(int(u16)), str(dep), str(sc.width), str(sc.height), repr(RATE)] + \
          [repr(float(v)) for v in sc.xform] + [str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    return np.fromfile(out, np.float32).reshape(sc.height, sc.width, 4)


def _scene(O, data):
    sc = O.Scene(data)
    sc.tf_mode = 1
    sc.tf_vg = O.copy_scale(U.fine_table(), RATE)       # renderVolume's copyScale(rate / gamma)
    sc.xform = O.rotation((1, 1, 0), 30)
    sc.width = sc.height = 40
    sc.steps, sc.sample_rate = 0, RATE
    return sc


def test_driver_is_built():
    assert os.path.exists(EXE), "build with __graft_entry__.build()"


@pytest.mark.gpu
def test_a_ushort_data_set_from_disk_keeps_its_sixteen_bits(tmp_path, O):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import volume_files as VF
    native, trex = _dataset(tmp_path)
    q16 = U.quantize_file16(native)
    assert np.array_equal(q16, native)                  # (the identity: the file spans 0..65535)
    sc16 = _scene(O, U.decode_u16(q16[..., None]))
    sc8 = _scene(O, np.ascontiguousarray(VF.quantize(native.astype(np.float64).ravel()).reshape(native.shape))[..., None])
    ref16, ref8 = sc16.render(), sc8.render()
    assert ref16[..., 3].max() > 0.05 and np.abs(ref16 - ref8).max() >= 1e-2, "vacuous: 8 bits render the same frame"
    got16 = _run(tmp_path, trex, True, sc16, "f16.f32")
    got8 = _run(tmp_path, trex, False, sc16, "f8.f32")
    e16, e8 = np.abs(got16 - ref16).max(), np.abs(got8 - ref8).max()
    print("from disk: 16-bit load against the checker %.3g; the default 8-bit load against its checker frame %.3g" % (e16, e8))
    assert e16 <= U.TOL, e16
    assert e8 <= U.TOL, e8                               # the switch off: the reference's 8-bit path, unchanged
