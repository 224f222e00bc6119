"""The data probe of a RESIDENT time step (smk.h smk_probe_step): the 2 x 2 x 2 corner voxels of a cell fetched from the
context's packed voxels must be the uploaded arrays' values exactly -- every voxel layout, with and without normals, at
the volume's borders, on shards (a rank answers for what its stored box holds), for blended and non-current steps -- and
the host-side mirror (HipVolumeRenderer::hist2DStep / probeStep, driven by tests/host/step_hist_main) must give
smktf::probe_sample's and hist2D()'s bytes on 8-bit data."""
import os
import subprocess

import numpy as np
import pytest

import _step_hist_ref as S
import _tblend_ref as T
from _layouts import stored_box
from _step_gpu import context, ring

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "step_hist_main")
NX, NY, NZ = S.DIMS
LAYOUTS = [(d, n) for d, top in (("u8", 4), ("u16", 3), ("f32", 4)) for n in range(1, top + 1)]


def cells():
    """200 random cells, the volume's eight corner cells, and cells with a coordinate of -1 and of N - 1 (not answered)"""
    rng = np.random.default_rng(23)
    c = [rng.integers(0, (NX - 1, NY - 1, NZ - 1)) for _ in range(200)]
    c += [(x, y, z) for z in (0, NZ - 2) for y in (0, NY - 2) for x in (0, NX - 2)]
    for a in range(3):
        for v in (-1, S.DIMS[a] - 1, S.DIMS[a], -2 ** 31, 2 ** 31 - 1):
            p = [5, 6, 7]
            p[a] = v
            c.append(tuple(p))
    return np.array(c, np.int64).astype(np.int32)


def same(got, want, what):
    for name, g, w in zip(("raw", "nrm", "ok"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if name == "raw":
            g, w = g.view(np.uint32), w.view(np.uint32)        # bit for bit
        assert np.array_equal(g, w), "%s: %s differs in %d places" % (what, name, int((g != w).sum()))


# ---- 1. random and border cells

@pytest.mark.parametrize("normals", [True, False])
@pytest.mark.parametrize("dtype, nelts", LAYOUTS)
def test_cells_of_every_layout(gpu_renderer_factory, dtype, nelts, normals):
    data, grad = S.volume(dtype, nelts)
    grad = grad if normals else None
    cs = cells()
    want = S.probe(data, grad, cs)
    assert want[2].sum() == 208 and not want[2][208:].any() and want[0][want[2]].any()
    if dtype == "f32" and nelts == 4:
        assert normals or (want[1][want[2]] == 128).all()   # (separate normals when there are any)
    R = context(gpu_renderer_factory, data, grad)
    try:
        same(R.probe_step(cs), want, "all cells")
        same(R.probe_step(cs[:1]), [w[:1] for w in want], "one cell")
    finally:
        R.close()


def test_refusals(gpu_renderer_factory, smk):
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match="smk_probe_step: no volume"):
            R.probe_step([(1, 1, 1)])
    finally:
        R.close()
    data, grad = S.volume("u8", 2)
    R = context(gpu_renderer_factory, data, grad)
    try:
        with pytest.raises(smk.SmkError, match="time step 3 is not cached"):
            R.probe_step([(1, 1, 1)], step=3)
        with pytest.raises(smk.SmkError, match="0 cells"):
            R.probe_step(np.zeros((0, 3), np.int32))
        with pytest.raises(smk.SmkError, match="65537 cells"):
            R.probe_step(np.zeros((65537, 3), np.int32))
        c = np.zeros((1, 3), np.int32)
        assert R.L.smk_probe_step(R.ctx, -1, c.ctypes.data, 1, None, None, None) != 0
        assert b"must be given" in R.L.smk_last_error(R.ctx)
        big = np.tile(cells()[:128], (512, 1))              # the most one call takes
        assert len(big) == 65536
        raw, nrm, ok = R.probe_step(big)
        want = S.probe(data, grad, big[:128])
        same((raw[-128:], nrm[-128:], ok[-128:]), want, "65536 cells")
    finally:
        R.close()


# ---- 2. shards

@pytest.mark.parametrize("dtype", ["u8", "f32", "u16"])
@pytest.mark.parametrize("nranks, halo", [(2, 1), (4, 3), (8, 1), (8, 3)])
def test_shards(gpu_renderer_factory, dtype, nranks, halo):
    data, grad = S.volume(dtype, 3)
    cs = cells()
    whole = S.probe(data, grad, cs)
    answered = np.zeros(len(cs), int)
    for rank in range(nranks):
        box = stored_box(S.DIMS, rank, nranks, dtype != "f32", halo)
        want = S.probe(data, grad, cs, box)
        R = context(gpu_renderer_factory, data, grad, shard=(rank, nranks), halo=halo)
        try:
            got = R.probe_step(cs)
        finally:
            R.close()
        same(got, want, "rank %d of %d, halo %d" % (rank, nranks, halo))
        ok = got[2]
        same([g[ok] for g in got], [w[ok] for w in whole], "a rank that answers agrees with the whole volume")
        answered += ok
    assert np.array_equal(answered > 0, whole[2])           # every in-volume cell is answered by some rank
    assert answered.max() > 1 and (answered[whole[2]] < nranks).any()


# ---- 3. blended and non-current steps

@pytest.mark.parametrize("dtype, nelts", [("u8", 3), ("f32", 3), ("u16", 3), ("f32", 4)])
def test_steps(gpu_renderer_factory, dtype, nelts):
    R, a, b = ring(gpu_renderer_factory, S.volume(dtype, nelts, 1), S.volume(dtype, nelts, 2))
    cs = cells()
    try:
        same(R.probe_step(cs, step=1), S.probe(b[0], b[1], cs), "a cached step that is not current")
        same(R.probe_step(cs), S.probe(a[0], a[1], cs), "the current step")
        R.blend_timesteps(0, 1, 0.3, 10)
        mid = T.blend(a[0], a[1], b[0], b[1], 0.3)
        same(R.probe_step(cs, step=10), S.probe(mid[0], mid[1], cs), "a blended step")
        R.select_timestep(10)
        same(R.probe_step(cs), S.probe(mid[0], mid[1], cs), "the blended step, current")
    finally:
        R.close()


# ---- 4. the host-side mirror

def _positions():
    rng = np.random.default_rng(31)
    p = (rng.random((120, 3)) * 1.2 - 0.1).astype(np.float32)          # inside and outside the volume
    edge = np.array([(0.0, 0.5, 0.5), (1.0 / NX, 0.5, 0.5), (0.999, 0.5, 0.5), ((NX - 1.5) / NX, 0.5, 0.5), (0.5, 0.5, (NZ - 0.5) / NZ),
                     (0.5, 1.5 / NY, 1.5 / NZ)], np.float32)
    return np.ascontiguousarray(np.concatenate([p, edge]))


def _drive(tmp_path, data, dmode):
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    vol, pos, out = tmp_path / "vol", tmp_path / "vpos.f32", tmp_path / "out"
    data.tofile(vol)
    _positions().tofile(pos)
    p = subprocess.run([EXE, str(vol), str(NX), str(NY), str(NZ), str(data.shape[-1]), str(int(data.dtype == np.uint16)), str(dmode),
                        str(pos), str(out)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    read = lambda ext, dt: np.fromfile(str(out) + ext, dt)
    return read, p.stderr


def test_adapter_on_8_bit_data(tmp_path):
    data = S.volume("u8", 3)[0]
    read, _ = _drive(tmp_path, data, 9)                                  # gluvvDataMode VGH
    hstep, h2d = read(".hstep", np.uint8), read(".h2d", np.uint8)
    assert hstep[0] == 1 and h2d[0] == 1
    assert np.array_equal(hstep, h2d)                                    # hist2D()'s bytes
    assert np.array_equal(hstep[1:].reshape(256, 256), S.finish(S.counts(data)))
    pstep, phost = read(".pstep", np.uint32).reshape(-1, 40), read(".phost", np.uint32).reshape(-1, 40)
    assert np.array_equal(pstep, phost)                                  # smktf::probe_sample on the host copy, byte for byte
    inside = pstep.view(np.float32)[:, 1]
    assert 20 < inside.sum() < len(inside) - 20 and pstep.view(np.float32)[inside > 0, 37:].any()


def test_adapter_on_16_bit_data(tmp_path):
    data = S.volume("u16", 2)[0]
    read, err = _drive(tmp_path, data, 1)                                # gluvvDataMode V1G
    hstep, h2d = read(".hstep", np.uint8), read(".h2d", np.uint8)
    assert hstep[0] == 1 and np.array_equal(hstep[1:].reshape(256, 256), S.finish(S.counts(data)))
    assert h2d[0] == 0 and not h2d.any() and "not implemented for 16-bit voxels" in err   # hist2D() as it was
    # the probe: corners = (float)((255 * (v / 65535)) / 255), in double
    rec = read(".pstep", np.float32).reshape(-1, 40)
    pos = _positions()
    seen = 0
    for r, p in zip(rec, pos):
        cell = [int(np.float32(p[a]) * np.float32(S.DIMS[a])) for a in range(3)]
        inside = all(1 <= cell[a] <= S.DIMS[a] - 2 for a in range(3))
        assert r[0] == 1 and bool(r[1]) == inside and (list(r[2:5]) == cell or not inside)
        if not inside:
            assert not r[5:].any()
            continue
        seen += 1
        want = np.zeros((8, 3), np.float32)
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    v = data[cell[2] + i, cell[1] + j, cell[0] + k].astype(np.float64)
                    want[i * 4 + j * 2 + k, :2] = ((255.0 * (v / 65535.0)) / 255.0).astype(np.float32)
        assert np.array_equal(r[5:29].reshape(8, 3), want)
    assert seen > 20
