"""Every translation unit of the slice-ring kernel's instances (smk_slab.h slab_inst_part, parts 0..7) on every workgroup
shape (option tile 5 / 20 / 4: 8+2, 10+2 and 12+4 waves): one small frame each, forced onto the kernel, against the checker
of the test that owns the frame kind, at that test's tolerance.  Where the instance table (tests/host/slab_inst_main) says the
frame's instance is not built, the kernel must decline with the table's reason -- and render on the same shape without brick
flags if that instance is built."""
import functools
import os
import subprocess

import numpy as np
import pytest

import _layouts as L
import _nv20_shadow_ref as N
import _u16_ref as U
from _scenes import make_scene, push_scene
from test_gpu_occlusion import VIEW, _blocky_levels, _checker_occluded, _depth_rule
from test_shadow_witness import compare

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4                                     # (test_gpu_slab.py, test_gpu_shadow.py, test_gpu_occlusion.py, _u16_ref.TOL)
TILES = {5: (8, 2), 20: (10, 2), 4: (12, 4)}   # option tile -> consumer + loader waves
N3, SIZE, STEPS = 32, 64, 64
LIGHT = (3, 4, -3)


@pytest.fixture(scope="module")
def R(gpu_renderer_factory):
    r = gpu_renderer_factory()
    yield r
    r.close()


@pytest.fixture(autouse=True)
def _restore(R):
    yield
    for k, v in (("kernel", 0), ("tile", 0), ("bricks", 1), ("shadow_look", 0)):
        R.set_option(k, v)
    R.set_shadow(0)


@functools.lru_cache(maxsize=None)
def _table():
    """key (dt, sh, perm, nw, nl, diag, tf, br, shd, occ, nvl) -> ("built", part) or ("missing", reason)"""
    out = subprocess.run([os.path.join(ROOT, "tests", "host", "slab_inst_main")], capture_output=True, text=True, check=True).stdout
    t = {}
    for line in out.splitlines():
        w = line.split(" ", 11)
        t[tuple(int(x) for x in w[:11])] = ("built", int(w[11].split()[1])) if w[11].startswith("built ") else ("missing", w[11])
    return t


# ---- one frame kind per part: its scene, its reference (computed once, read-only), how to push and check it.  Each
# returns (key fields dt, sh, tf, shd, occ, nvl; push(R); render(R) -> what check takes; check(got))

def _plain(f32):
    sc = make_scene("cfg3", n=N3, size=SIZE, steps=STEPS, pose="rot", f32=f32, shade=1)
    ref = sc.render()
    assert ref[..., 3].max() > 0.05

    def check(got):
        assert np.abs(got - ref).max() <= TOL
    return (int(f32), 1, 1, 0, 0, 0), lambda R: push_scene(R, sc), lambda R: R.render(), check


def _shadow():
    sc = make_scene("cfg3", n=N3, size=SIZE, steps=STEPS, f32=True, shade=1)
    sc.light_pos, sc.shadow = LIGHT, (64, 0.5)
    ref, refL = sc.render_shadow()
    assert ref[..., 3].max() > 0.05 and refL[..., 3].max() > 0.05

    def check(got):
        assert np.abs(got[1] - refL).max() <= TOL and np.abs(got[0] - ref).max() <= TOL
    return (1, 1, 1, 1, 0, 0), lambda R: push_scene(R, sc), lambda R: (R.render(), R.light_buffer()), check


def _occluded():
    sc = make_scene("tf3d", n=N3, size=SIZE, steps=STEPS, f32=False, shade=1)
    state = {}

    def push(R):
        push_scene(R, sc)
        if not state:    # (the occluder's levels come from the context's own plane depths: test_gpu_occlusion.py)
            levels, idx = _blocky_levels(R, sc, np.random.default_rng(5))
            state["zs"] = levels[idx].astype(np.float32)
            state["ref"], state["rd"] = _checker_occluded(sc, levels, idx, 0)
            assert state["ref"][..., 3].max() > 0.05 and np.isfinite(state["rd"]).mean() > 0.05

    def check(got):
        assert np.abs(got[0] - state["ref"]).max() <= TOL
        _depth_rule(state["rd"], got[1])
    return (0, 1, 2, 0, 1, 0), push, lambda R: R.render(depth=True, scene_depth=state["zs"], scene_depth_kind=VIEW), check


def _occluded_shadow():
    """(test_gpu_occlusion.py::test_shadows_occlude_the_eye_pass_only) the left half in front of the volume, the right behind"""
    sc = make_scene("cfg3", n=N3, size=SIZE, steps=STEPS, f32=True, shade=1)
    sc.light_pos, sc.shadow = LIGHT, (64, 0.75)
    ref, refL = sc.render_shadow()
    assert ref[:, SIZE // 2:, 3].max() > 0.05
    zs = np.full((SIZE, SIZE), 1e3, np.float32)
    zs[:, : SIZE // 2] = 1e-3

    def check(got):
        assert not got[0][:, : SIZE // 2].any()
        assert np.abs(got[0][:, SIZE // 2:] - ref[:, SIZE // 2:]).max() <= TOL and np.abs(got[1] - refL).max() <= TOL
    return (1, 1, 1, 1, 1, 0), lambda R: push_scene(R, sc), lambda R: (R.render(scene_depth=zs), R.light_buffer()), check


def _nv20():
    """(test_gpu_shadow_nv20.py) float voxels: their 10+2-wave instances with brick flags are the ones left out"""
    sc, w = N.witness_of("slab-parts", lambda: N.nv20_scene("cfg3", "behind", "back", amb=0.5, f32=True, shade=2, n=N3, size=SIZE, steps=STEPS))

    def push(R):
        push_scene(R, sc)
        R.set_shading("nv20", sc.light_pos, sc.eye, sc.at, sc.xform, sc.intens, sc.amb)
        R.set_option("shadow_look", 1)
    return (1, 2, 1, 1, 0, 1), push, lambda R: (R.render(), R.light_buffer()), lambda got: compare(got[0], got[1], w)


def _u16(shadow):
    k = U.case(3, "2d3", shade=1, view="rot", window=(SIZE, SIZE), dims=(N3, N3, N3))
    sc = k.sc
    sc.steps = STEPS
    if shadow:
        sc.light_pos, sc.shadow = L.SHADOW_LIGHT, L.SHADOW
        ref, refL = sc.render_shadow()
        assert ref[..., 3].max() > 0.05 and refL[..., 3].max() > 0.05

        def check(got):
            assert np.abs(got[1] - refL).max() <= U.TOL and np.abs(got[0] - ref).max() <= U.TOL
        return (2, 1, 1, 1, 0, 0), lambda R: U.push(R, k), lambda R: (R.render(), R.light_buffer()), check
    ref = sc.render()
    assert ref[..., 3].max() > 0.05

    def check(got):
        assert np.abs(got - ref).max() <= U.TOL
    return (2, 1, 1, 0, 0, 0), lambda R: U.push(R, k), lambda R: R.render(), check


KINDS = [lambda: _plain(False), lambda: _plain(True), _shadow, _occluded, _occluded_shadow, _nv20, lambda: _u16(False), lambda: _u16(True)]


@functools.lru_cache(maxsize=None)
def _kind(part):
    return KINDS[part]()


@pytest.mark.parametrize("tile", sorted(TILES, key=TILES.get))
@pytest.mark.parametrize("part", range(8))
def test_every_part_on_every_shape(R, smk, part, tile):
    (dt, sh, tf, shd, occ, nvl), push, render, check = _kind(part)
    nw, nl = TILES[tile]
    push(R)
    R.set_option("kernel", 2)
    R.set_option("tile", 5)
    render(R)                                   # (8+2 waves has every instance: the frame's slice axis, and its brick flags)
    assert R.last_frame_info()[0] == 2
    perm, flags = int(R.stat("slab_plan_perm")), int(R.stat("slab_plan_bricks"))
    key = lambda br: (dt, sh, perm, nw, nl, 0, tf, br, shd, occ, nvl)   # noqa: E731
    R.set_option("tile", tile)
    want = _table()[key(1 if occ else flags)]
    if want[0] == "missing":
        with pytest.raises(smk.SmkError) as e:
            render(R)
        assert "not applicable: " + want[1] in str(e.value), str(e.value)
        if _table()[key(0)][0] != "built":
            return
        R.set_option("bricks", 0)               # (the same shape without brick flags has its instance)
    got = render(R)
    assert R.last_frame_info()[0] == 2
    assert (int(R.stat("slab_plan_nw")), int(R.stat("slab_plan_nl"))) == (nw, nl)
    assert _table()[key(1 if occ else int(R.stat("slab_plan_bricks")))] == ("built", part)
    check(got)
