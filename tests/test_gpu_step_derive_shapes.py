"""Derived steps (smk.h smk_derive_timestep, smk_upload_timestep_scalar_device) against the CPU checker alone -- O.make_vgh,
O.normals_vgh, _prep_f32_ref.normals_f32 and _u16_ref.quantize_u16 through tests/_step_derive_ref.py derive -- where
tests/test_gpu_step_derive.py compares with the recipe's device entries, which share smk_prep_device.h with the derive
kernels.  Every scalar type into every ring, float scalars that are signed or lie beyond the reference's +-1e8 seeds, volumes
at the edges of the kernels' 32 x 8 x 8 tiles, and a volume of more tiles than the stats pass has workgroups.  Every scalar is
finite (the checker's MAX/MIN macros give a NaN no contract); every comparison is equality of bits.  The volumes are qualified
in tests/test_step_derive_cpu.py."""
import functools

import numpy as np
import pytest

import _step_derive_ref as V
from _gpu_mem import dev_ptr as dev
from _step_gpu import recipe_download, same_bits as same, series

pytestmark = pytest.mark.gpu
IDS = dict(ids=lambda d: "x".join(map(str, d)) if isinstance(d, tuple) else None)


def step_of(s, ring):
    """a step (data, normals) of a ring of type `ring` whose channel 0 is the scalar s; what it holds besides is never read"""
    assert s.dtype == V.NP[ring]
    nz, ny, nx = s.shape
    data = np.zeros((nz, ny, nx, 3), s.dtype)
    data[..., 0] = s
    data[..., 1] = s[::-1]
    return data, np.full((nz, ny, nx, 3), 7, np.uint8)


def holder(factory, dims, ring):
    """a context whose series has `dims` and voxels of type `ring`: step 0 is current, one slot is free"""
    return series(factory, (step_of(V.as_type(V.scalar(0, dims), ring), ring),), cap=2)


def check(got, want, what):
    same(got[0], want[0], what + ": data against the checker")
    same(got[1], want[1], what + ": normals against the checker")


# ---- 1. every scalar type into every ring, each flag with each value of the other

@pytest.mark.parametrize("ring", V.RINGS)
@pytest.mark.parametrize("name", V.SCALARS)
def test_scalar_form_against_the_checker(gpu_renderer_factory, O, name, ring):
    dims = V.SMALL
    s = V.typed(V.scalar(1, dims), name)
    R = holder(gpu_renderer_factory, dims, ring)
    try:
        ps, keep = dev(s)
        for compat, blur in V.ALL_CASES:
            R.upload_timestep_scalar_device(4, ps, V.CODE[V.KIND[name]], dims, compat, blur)
            assert R.timesteps() == (0, [0, 4])
            got = R.download_timestep(4)
            assert got[0][1:-1, 1:-1, 1:-1].any(axis=(0, 1, 2)).all() and (got[1] != 128).any()
            check(got, V.downloaded(*V.derive(O, s, ring, compat, blur)), "%s into %s, compat %d, blur %d" % (name, ring, compat, blur))
    finally:
        R.close()


# (the source of smk_derive_timestep is channel 0 of the ring's packed voxels: a scalar of the ring's own type)
SOURCES = [(V.KIND[name], name) for name in V.SCALARS]


@pytest.mark.parametrize("ring, name", SOURCES)
def test_derive_timestep_against_the_checker(gpu_renderer_factory, O, ring, name):
    dims = V.SMALL
    s = V.typed(V.scalar(1, dims), name)
    src = step_of(s, ring)
    R = series(gpu_renderer_factory, (src,), cap=2)
    try:
        for compat, blur in V.ALL_CASES:
            R.derive_timestep(0, 1, compat, blur)
            assert R.timesteps() == (0, [0, 1])
            got = R.download_timestep(1)
            assert got[0][1:-1, 1:-1, 1:-1].any(axis=(0, 1, 2)).all() and (got[1] != 128).any()
            check(got, V.downloaded(*V.derive(O, s, ring, compat, blur)), "%s in a %s ring, compat %d, blur %d" % (name, ring, compat, blur))
        same(R.download_timestep(0)[0], V.downloaded(*src)[0], "the source, afterwards")
    finally:
        R.close()


# ---- 2. tile edges: whole tiles, one voxel short of them, one and two voxels past them

@pytest.mark.parametrize("ring", V.RINGS)
@pytest.mark.parametrize("dims", V.TILE_SHAPES, **IDS)
def test_tile_edges_against_the_checker(gpu_renderer_factory, O, dims, ring):
    """both forms on full-range noise: smk_derive_timestep from the ring's packed voxels (nx 31 and 33 put the pad column of
    8-byte voxels at a tile's end and alone in the next tile) and the scalar form from a dense u8 scalar, plain and blurred
    normals.  For one ring per shape the recipe's upload is compared too"""
    s8 = V.noise(dims)
    s = V.typed(s8, ring)
    src = step_of(s, ring)
    R = series(gpu_renderer_factory, (src,), cap=2)
    try:
        p8, keep = dev(s8)
        for compat, blur in V.TILE_CASES:
            R.derive_timestep(0, 1, compat, blur)
            got = R.download_timestep(1)
            check(got, V.downloaded(*V.derive(O, s, ring, compat, blur)), "derive_timestep, blur %d" % blur)
            if ring == V.RINGS[V.TILE_SHAPES.index(dims) % 3] and blur:
                want = recipe_download(gpu_renderer_factory, R, s, ring, compat, blur)
                same(got[0], want[0], "data against the recipe")
                same(got[1], want[1], "normals against the recipe")
            R.upload_timestep_scalar_device(1, p8, V.CODE["u8"], dims, compat, blur)
            check(R.download_timestep(1), V.downloaded(*V.derive(O, s8, ring, compat, blur)), "the scalar form, blur %d" % blur)
        same(R.download_timestep(0)[0], V.downloaded(*src)[0], "the source, afterwards")
    finally:
        R.close()


# ---- 3. more tiles than the stats pass has workgroups: 5 x 377 x 361 voxels are 1 x 48 x 46 tiles
assert V.THIN == (5, 377, 361)
assert 48 * 46 > 2048                                       # DV_STATS_BLOCKS (csrc/smk_step_derive.hip): 160 workgroups take a second tile


@functools.lru_cache(maxsize=None)
def thin(kind):
    s = V.as_type(V.thin_scalar(), kind)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def thin_want(O, kind, ring, compat, blur):
    """the checker's step of the thin scalar: the extremes of the data, and G and H beside them, lie in tiles that only a
    second turn of the stats loop visits (tests/test_step_derive_cpu.py: without it 98 % of the bytes change)"""
    want = V.downloaded(*V.derive(O, thin(kind), ring, compat, blur))
    v = want[0][..., 0]
    assert v[V.PLANT[0]] == 0 and v[V.PLANT[1]] == (255 if ring == "u8" else 1)
    for a in want:
        a.setflags(write=False)
    return want


THIN_CASE = {"u8": (1, 1), "f32": (0, 1)}                   # (compat, blur) by the scalar's type


@pytest.mark.parametrize("ring", ["u8", "f32"])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_thin_volume_scalar_form_against_the_checker(gpu_renderer_factory, O, kind, ring):
    compat, blur = THIN_CASE[kind]
    R = series(gpu_renderer_factory, (step_of(np.zeros(V.THIN[::-1], V.NP[ring]), ring),), cap=2)
    try:
        ps, keep = dev(thin(kind))
        R.upload_timestep_scalar_device(1, ps, V.CODE[kind], V.THIN, compat, blur)
        got = R.download_timestep(1)
    finally:
        R.close()
    check(got, thin_want(O, kind, ring, compat, blur), "%s into %s" % (kind, ring))


@pytest.mark.parametrize("ring", ["u8", "f32"])
def test_thin_volume_derive_timestep_against_the_checker(gpu_renderer_factory, O, ring):
    compat, blur = THIN_CASE[ring]
    R = series(gpu_renderer_factory, (step_of(np.array(thin(ring)), ring),), cap=2)
    try:
        R.derive_timestep(0, 1, compat, blur)
        got = R.download_timestep(1)
    finally:
        R.close()
    check(got, thin_want(O, ring, ring, compat, blur), "a %s ring" % ring)
