"""The time-step cache without a GPU: the new entries are declared and bound, and a .trex series' fields and brick files
come through VolumeFiles (parse_trex / load_trex) as the host needs them to step through the series."""
import os
import re
import subprocess

import numpy as np
import pytest

from _trex_series import write_series

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
NEW = ["smk_set_timestep_cache", "smk_upload_timestep", "smk_upload_timestep_device", "smk_select_timestep",
       "smk_get_timesteps"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smk.h")).read(), flags=re.S)


def test_new_entries_are_declared_bound_and_exported(smk):
    src = _header()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in smk.ABI_SYMBOLS, name
    L = smk.load_library()
    for name in NEW:
        assert hasattr(L, name), name
    for name in ("set_timestep_cache", "upload_timestep", "upload_timestep_device", "select_timestep", "timesteps"):
        assert callable(getattr(smk.Renderer, name)), name


def test_new_declarations_parse_as_c():
    """the header stays plain C: a C compiler accepts it and the prototypes it declares"""
    probe = "#include \"smk.h\"\nint (*p0)(smk_ctx *, int) = smk_set_timestep_cache;\n" \
            "int (*p1)(smk_ctx *, int, const smk_volume_desc *, int, int, smk_dtype, smk_datamode) = smk_upload_timestep;\n" \
            "int (*p2)(smk_ctx *, int, const smk_volume_desc *, int, int, smk_dtype, smk_datamode, void *) = smk_upload_timestep_device;\n" \
            "int (*p3)(smk_ctx *, int) = smk_select_timestep;\n" \
            "int (*p4)(smk_ctx *, int *, int *, int, int *) = smk_get_timesteps;\n"
    p = subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=probe, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_trex_series_fields_round_trip(tmp_path):
    files_main = os.path.join(HOST, "files_main")
    ts_main = os.path.join(HOST, "timestep_main")
    for exe in (files_main, ts_main):
        assert os.path.exists(exe), "%s is not built (__graft_entry__.build())" % exe
    rng = np.random.default_rng(7)
    steps = [rng.integers(0, 256, (10, 12, 16), dtype=np.uint8) for _ in range(3)]
    trex = write_series(str(tmp_path), steps)
    p = subprocess.run([files_main, "parse", trex], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert "tsteps=3 3 5" in p.stdout and "cache=2" in p.stdout
    # every step's bricks, read as readAll(timestep) reads them
    for k, v in enumerate(steps):
        out = str(tmp_path / ("step%d.u8" % k))
        p = subprocess.run([files_main, "load", trex, str(3 + k), out], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        assert np.array_equal(np.fromfile(out, np.uint8), v.reshape(-1))
    # ... and the MetaVolume series fields load_trex fills
    p = subprocess.run([ts_main, "info", trex], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    rows = p.stdout.strip().splitlines()
    assert len(rows) == 3
    for k, row in enumerate(rows):
        assert "step=%d tsteps=3 tstart=3 tstop=5 tstepCache=2 currentTStep=%d" % (3 + k, 3 + k) in row
        assert row.endswith("series.%04d.00" % (3 + k))


def test_timestep_driver_fails_loudly_without_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    ts_main = os.path.join(HOST, "timestep_main")
    assert os.path.exists(ts_main), "%s is not built (__graft_entry__.build())" % ts_main
    trex = write_series(str(tmp_path), [np.zeros((10, 12, 16), np.uint8)] * 2)
    p = subprocess.run([ts_main, "draw", trex, "8", "8", "1", "3,4", str(tmp_path / "f")], capture_output=True, text=True)
    assert p.returncode == 3 and "no HIP device" in p.stderr
