"""The cases of tests/_layouts.py qualified on the CPU checker alone: what keeps tests/test_gpu_layouts.py from passing
vacuously.  Every frame shows something; the fourth channel, the third axis, the normals and the data mode each move the
checker's frame by a hundred tolerances where a case says they matter, and by nothing where it says they do not; the
bricks tile, are uneven and lie across the shards' boxes; the slice quads stay under the existing edge cap in the
reference alone.  No GPU, no product code."""
import numpy as np
import pytest

import _layouts as L

SHOWS = 0.05        # test_gpu_parity.py::_check
MARGIN = 1e-2       # 100 x TOL


def _shows(f):
    return f[..., 3].max() > SHOWS


@pytest.fixture(scope="module")
def frames():
    cache = {}

    def get(c):
        if c not in cache:
            cache[c] = L.case_scene(c).render()
        return cache[c]
    return get


CASES = L.channel_cases()


def test_the_case_list_is_what_the_gpu_tests_expect():
    assert len(CASES) == 16 and len(set(CASES)) == 16
    for f32 in (False, True):
        for n in (1, 2, 3, 4):
            assert any(c[:3] == (n, f32, "2d" if n < 3 else "2d3") for c in CASES)
            assert any(c[:3] == (n, f32, "3d") for c in CASES) == (n >= 3)
        assert sum(c[1] == f32 and c[3] == 2 for c in CASES) == 1      # NV20 shading, one case of each type
    assert {c[4] for c in CASES} == {"rot", "x+", "x-", "close"}
    for w, h in L.WINDOWS + tuple(w for w, _ in L.SLICE_CASES if w != (16, 16)):
        assert w % 16 or h % 16
    assert L.MODES.index("VGH") == 9 and len(L.MODES) == 13 and set(L.THIRD) <= set(L.MODES) and len(L.THIRD) == 7
    # the wide pair is sized from the two planners' conditions: the column-stream kernel drops the alpha row above 1024
    # texels, the slice-ring kernel above 2048
    assert 1024 < L.tf_third(*L.WIDE).shape[1] <= 2048 and L.tf_ramp(*L.WIDE).shape == L.tf_third(*L.WIDE).shape


@pytest.mark.parametrize("c", CASES, ids=L.case_id)
def test_channel_cases(frames, c):
    sc = L.case_scene(c)
    f = frames(c)
    assert _shows(f)
    assert sc.third_axis == (1 if sc.nelts >= 3 and sc.tf_mode == 1 else 0)
    if sc.nelts == 4 and sc.tf_mode == 1:
        d = sc.data.copy()
        d[..., 3] = 0
        assert np.abs(L.with_data(sc, d).render() - f).max() >= MARGIN, "channel 3 does not show"
        d = sc.data.copy()
        d[..., [2, 3]] = d[..., [3, 2]]
        assert np.abs(L.with_data(sc, d).render() - f).max() >= MARGIN, "channels 2 and 3 could be swapped unseen"
    if sc.third_axis:
        sc.third_axis = 0
        assert np.abs(sc.render() - f).max() >= MARGIN
        sc.third_axis = 1
    assert sc.shade_mode and sc.grad is not None
    sc.shade_mode = 0
    plain = sc.render()
    if sc.nelts == 1:
        # the R8k look blends the lit colour in by the SECOND channel (oracle/smk_oracle.c: LERP by G), which a one-channel
        # volume does not have: lit and unlit frames are the same numbers, and that is the property
        assert c[3] == 1 and np.array_equal(plain, f)
    else:
        assert np.abs(plain - f).max() >= MARGIN


def test_the_third_axis_tables_vary_along_both_axes():
    for size in ((256, 256), L.WIDE):
        a = L.tf_third(*size)[..., 3].astype(int)
        # (a product of two waves: constant along t only in the few columns where the wave along s passes 0)
        assert np.median(np.ptp(a, axis=0)) > 40 and np.median(np.ptp(a, axis=1)) > 40
    r = L.tf_ramp()
    assert r[0, :, 3].min() > 0, "the g = 0 row, all a one-channel volume samples, must show"


@pytest.mark.parametrize("nelts", L.RULE_VOLUMES + (2,))
def test_the_data_mode_rule(nelts):
    """NV20VolRen3D.cpp:686-693: seven of the thirteen modes multiply the third-axis alpha in, the other six do not -- and a
    two-channel volume has no third channel to look up, whatever its mode"""
    none = L.rule_scene(nelts, "V1", second=False).render()
    assert _shows(none)
    for m in L.MODES:
        sc = L.rule_scene(nelts, m)
        assert sc.tf_h is not None
        assert sc.third_axis == (1 if m in L.THIRD and nelts >= 3 else 0)
        f = sc.render()
        if sc.third_axis:
            assert np.abs(f - none).max() >= MARGIN and _shows(f)
        else:
            assert np.array_equal(f, none)
    assert [m for m in L.MODES if m not in L.THIRD] == ["V1", "V1G", "V2", "VGH_VG", "VGH_V", "UNKNOWN"]


@pytest.mark.parametrize("f32", [False, True])
def test_without_normals_shading_changes_nothing(f32):
    sc = L.no_normals_scene(f32)
    assert sc.grad is None and sc.shade_mode == 1
    f = sc.render()
    sc.shade_mode = 0
    assert _shows(f) and np.array_equal(f, sc.render())
    lit = L.scene(3, f32, "2d3", shade=1, view="rot", steps=44)
    assert np.abs(lit.render() - f).max() >= MARGIN      # (with the normals the same request does shade)


# the boxes the contexts of section d keep, stated: (rank, nranks, u8) -> (origin, size).  Region = the halves of
# sortlast.shard_region (x at 10, y at 6), + 1 halo voxel, u8 rows evened out in x and y
BOXES = {
    (0, 1, True): ((0, 0, 0), (22, 14, 7)), (0, 1, False): ((0, 0, 0), (21, 13, 7)),       # u8: a pad column in x and in y
    (0, 2, True): ((0, 0, 0), (12, 14, 7)), (0, 2, False): ((0, 0, 0), (11, 13, 7)),       # 0..10 + halo = 11 -> 12
    (1, 2, True): ((9, 0, 0), (12, 14, 7)), (1, 2, False): ((9, 0, 0), (12, 13, 7)),
    (0, 4, True): ((0, 0, 0), (12, 8, 7)), (0, 4, False): ((0, 0, 0), (11, 7, 7)),
    (3, 4, True): ((9, 5, 0), (12, 8, 7)), (3, 4, False): ((9, 5, 0), (12, 8, 7)),
}


def test_stored_boxes(smk):
    from simian_spacemonkey_amd import sortlast
    assert sortlast.shard_region(L.DIMS_ODD, 0, 2) == ((0, 0, 0), (10, 13, 7))
    assert sortlast.shard_region(L.DIMS_ODD, 3, 4) == ((10, 6, 0), (21, 13, 7))
    for (rank, world, u8), box in BOXES.items():
        assert L.stored_box(L.DIMS_ODD, rank, world, u8) == box, (rank, world, u8)
    assert set(BOXES) == {(r, w, u) for r, w in L.PACK_SHARDS for u in (True, False)}


@pytest.mark.parametrize("nelts,f32", L.PACK_LAYOUTS)
def test_packing_cases(smk, nelts, f32):
    sc = L.pack_scene(nelts, f32)
    assert sc.dims == L.DIMS_ODD and _shows(sc.render())
    fs = [np.float32(f) for f in sc.fsize]
    for grid in L.PACK_GRIDS:
        bs = L.bricks(sc.dims, sc.fsize, grid)
        assert len(bs) == grid[0] * grid[1] * grid[2]
        seen = np.zeros(sc.dims[::-1], int)
        for ipos, isize, fpos, fsz in bs:
            seen[ipos[2]:ipos[2] + isize[2], ipos[1]:ipos[1] + isize[1], ipos[0]:ipos[0] + isize[0]] += 1
        assert (seen == 1).all(), "the bricks do not tile the volume"
        for a in range(3):
            sizes = {b[1][a] for b in bs}
            assert (len(sizes) > 1) == (grid[a] > 1), "every axis that is cut is cut unevenly"
            # the extent the product derives -- the largest fPos + fSize in float arithmetic -- is the single brick's
            assert max(np.float32(np.float32(b[2][a]) + np.float32(b[3][a])) for b in bs) == fs[a]
        o = L.shuffled(len(bs))
        assert o != sorted(o)
        for rank, world in L.PACK_SHARDS:
            if world == 1:
                continue
            box = BOXES[(rank, world, not f32)]
            rel = [L.brick_relation(b, box) for b in bs]
            assert "cut" in rel, (grid, rank, world)
            # (one cut in x cannot lie outside both halves' boxes: under (2, 2, 2) rank 1 of 2 has no brick to skip)
            assert ("out" in rel) == ((grid, rank, world) != ((2, 2, 2), 1, 2)), (grid, rank, world)
    for rank, world in L.PACK_SHARDS:                     # every shard's own frame shows something
        from simian_spacemonkey_amd import sortlast
        sc.region = sortlast.shard_region(sc.dims, rank, world)
        assert _shows(sc.render()), (rank, world)


def test_time_steps_differ():
    a, b = [s.render() for s in L.step_scenes()]
    assert _shows(a) and _shows(b) and np.abs(a - b).max() > MARGIN
    s0, s1 = L.step_scenes()
    assert not np.array_equal(s0.grad, s1.grad) and not np.array_equal(s0.data, s1.data)
    swapped = L.with_data(s0, s0.data, grad=s1.grad)      # step 0's voxels under step 1's normals: the normals show alone
    assert np.abs(swapped.render() - a).max() > MARGIN


@pytest.mark.parametrize("f32", [False, True])
def test_shadow_cases(f32):
    """the light and layout pair passes the qualification of test_gpu_shadow.py::_check (frame and light buffer show), the
    shadow term does something, and the fourth channel shows in the shadowed frame"""
    sc = L.shadow_scene(f32)
    f, lb = sc.render_shadow()
    assert _shows(f) and lb[..., 3].max() > SHOWS
    assert np.abs(f - sc.render()).max() >= MARGIN
    d = sc.data.copy()
    d[..., 3] = 0
    z, zl = L.with_data(sc, d).render_shadow()
    assert np.abs(z - f).max() >= MARGIN and np.abs(zl - lb).max() >= MARGIN


def test_wide_range_case():
    sc = L.wide_range_scene()
    assert sc.data.min() < -0.25 and sc.data.max() > 1.25
    f = sc.render()
    assert _shows(f) and np.abs(f - L.scene(3, True, "2d3", shade=1, view="rot", steps=44).render()).max() >= MARGIN


@pytest.mark.parametrize("window,name", L.SLICE_CASES, ids=lambda v: v if isinstance(v, str) else "%dx%d" % v)
@pytest.mark.parametrize("f32", [False, True])
def test_slice_quads(window, name, f32):
    sc = L.slice_scene(3, f32, window)
    base = sc.render()
    assert _shows(base), "the quad is drawn over a frame that is not empty"
    q = L.quads(sc)[name]
    for alpha in L.ALPHAS:
        want, edge = L.slice_reference(sc, base, q, alpha)
        inner = ~edge
        assert edge.sum() < 0.1 * inner.sum()           # test_host_adapter.py's cap, in the reference alone
        if name in L.NO_DRAW:
            assert np.array_equal(want, base.astype(np.float64)) and not edge.any()
        else:
            assert np.abs(want - base)[inner].max() > 0.05


def test_slice_volumes_reach_the_faces_and_differ_by_channel():
    """a clamped fetch outside the box returns a face voxel: those must not be 0, or the 'outside' quad and the quads that
    must not be drawn would add nothing either way; and channel 0 must differ from the channels beside it"""
    for f32 in (False, True):
        for nelts in (1, 3, 4):
            d = L.slice_scene(nelts, f32).data.astype(np.float64)
            assert d.shape[-1] == nelts
            for face in (d[0], d[-1], d[:, 0], d[:, -1], d[:, :, 0], d[:, :, -1]):
                assert face[..., 0].min() > (0.02 if f32 else 5)
            for e in range(1, nelts):
                assert np.abs(d[..., e] - d[..., 0]).mean() > (0.05 if f32 else 12)
    sc = L.slice_scene(3, False)
    base = sc.render()
    want, edge = L.slice_reference(sc, base, L.quads(sc)["outside"], 0.6)
    zero = L.slice_scene(3, False)
    d = zero.data.copy()
    d[[0, -1]] = 0
    d[:, [0, -1]] = 0
    d[:, :, [0, -1]] = 0
    w0, _ = L.slice_reference(L.with_data(zero, d), base, L.quads(sc)["outside"], 0.6)
    assert np.abs(w0 - want)[~edge].max() > 0.05         # the part of the quad outside the box shows the face voxels
