"""bench.py's two modes on one GPU, at a small size: a plain run carries the headline figures and what falls out of
the timed steps, nothing that takes frames or CPU time of its own; --full adds those after the timed steps and the
dump, so both modes hand out the same frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--volume", "96", "--size", "192", "--planes", "96"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
# what only --full may put on the line: each takes frames, volumes or CPU time beyond the timed steps
FULL_ONLY = ("samples", "without_brick_flags", "sortlast_check", "cpu_baseline", "north_star", "extra")


def _run(extra, dump):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SMK_BENCH_REHEARSE")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra + ["--dump-outputs", str(dump)]
    p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), np.load(os.path.join(str(dump), "frame.npy"))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_modes")
    # (the 1024^3 north star and the CPU checker's seconds stay out of the suite: the flags say so, --full does the rest)
    return _run([], d / "plain"), _run(["--full", "--no-north-star", "--no-cpu"], d / "full")


def test_plain_run_carries_the_headline_and_nothing_that_needs_runs_of_its_own(runs):
    out, frame = runs[0]
    for k in HEADLINE:
        assert k in out, k
    assert out["full"] is False and out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "Msamples/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(192 * 192 * 96 / (out["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)
    assert [k for k in FULL_ONLY if k in out] == []
    # ... while what the timed steps measured themselves stays on the line
    assert out["roofline"]["kernel_frames_timed"] == 3 and out["roofline"]["kernel_ms"] > 0
    assert out["slab_failures"] == 0
    assert frame.shape == (192, 192, 4) and frame[..., 3].max() > 0.05


def test_full_run_adds_the_secondary_figures_and_dumps_the_same_frame(runs):
    (plain, frame), (out, frame_full) = runs
    for k in HEADLINE:
        assert k in out, k
    assert out["full"] is True and out["metric"] == plain["metric"] and out["unit"] == plain["unit"]
    s = out["samples"]
    assert s["nominal"] == 192 * 192 * 96 and 0 < s["in_volume"] <= s["nominal"]
    assert out["without_brick_flags"]["frame_bit_identical_to_the_one_with_flags"] is True
    assert "cpu_baseline" not in out and "north_star" not in out     # --no-cpu, --no-north-star
    assert out["slab_failures"] == 0
    # the dump precedes everything --full adds: the same frame, up to the 2e-5 the project allows two marchers that
    # associate a ray's blend differently (auto mode settles on whichever measured faster in that process)
    assert np.abs(frame_full - frame).max() <= 2e-5
