"""The volumes of tests/test_gpu_step_merge.py, qualified on the references alone (tests/_step_merge_ref.py: the CPU checker's
mergeMV, _prep_f32_ref.merge_fields_f32, _u16_ref.quantize_u16) so that no GPU test can pass vacuously.  No GPU."""
import numpy as np
import pytest

import _prep_f32_ref as P
import _step_merge_ref as M
import _u16_ref as U


def quantised(ring, g):
    """the stored last channel of a float G in [0, 1] (for u8: the byte of the float quotient's double product)"""
    if ring == "u8":
        return (g.astype(np.float64) * 255.0).astype(np.int64).astype(np.uint8)
    return g if ring == "f32" else U.quantize_u16(g)


@pytest.mark.parametrize("dims", M.DIMS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("ring, nf", M.CASES)
def test_volumes_are_not_vacuous(O, ring, nf, dims):
    F = M.fields(ring, nf, dims)
    assert F.dtype == M.NP[ring] and F.shape == dims[::-1] + (nf,)
    mag = M.magnitude(F)
    assert np.isfinite(mag).all() and mag.max() > 0            # (the checker divides by the maximum)
    assert (mag[2:7, 3:8, 4:10][1:-1, 1:-1, 1:-1] == 0).all()  # the flat block: zero gradients, normal (128, 128, 128)
    data, nrm = M.merge(O, F)
    assert data.dtype == F.dtype and data.shape == F.shape[:3] + (nf + 1,) and nrm.shape == F.shape[:3] + (3,)
    assert np.array_equal(data[..., :nf].view(np.uint8), F.view(np.uint8)), "the fields are copied, on the border too"
    G = data[..., nf]
    assert len(np.unique(G)) > 60, "G takes many distinct values"
    assert (nrm != 128).any() and (nrm[0] == 128).all() and (nrm[:, 0] == 128).all() and (nrm[:, :, 0] == 128).all()
    assert not G[0].any() and not G[:, -1].any() and not G[:, :, -1].any() and F[0].any()   # G is 0 on the border, the fields are not
    # the source step's last channel and normals are not the merged ones
    sdata, snrm = M.source_step(F)
    assert not np.array_equal(sdata[..., nf], G) and not np.array_equal(snrm, nrm)
    if nf > 1:                                                   # every field counts: the gradient of field 0 alone differs
        assert not np.array_equal(M.merge(O, np.ascontiguousarray(F[..., :1]))[1], nrm)


def test_u8_restatement_is_the_checkers(O):
    """the float restatement of the summed gradient (the one the float rings use) gives the checker's bytes for u8 fields"""
    for nf in (1, 2, 3):
        F = M.fields("u8", nf, M.SMALL)
        data, nrm = M.merge(O, F)
        mag = M.magnitude(F)
        with np.errstate(all="ignore"):
            q = ((mag / mag.max()).astype(np.float32).astype(np.float64) * 255.0).astype(np.int64).astype(np.uint8)
        assert np.array_equal(q, data[..., nf])
        assert np.array_equal(P.normal_bytes(M.central_sum(F.astype(np.float32))), nrm)


def planted_volumes():
    out = []
    for ring in M.RINGS:
        out.append(("thin-" + ring, ring, lambda ring=ring: (M.thin_fields(ring), M.THIN_AT)))
        for dims in M.tile_shapes(ring):
            out.append(("%s-%s" % (ring, "x".join(map(str, dims))), ring, lambda ring=ring, dims=dims: M.planted_last(ring, 2, dims)))
    return out


@pytest.mark.parametrize("name, ring, make", planted_volumes(), ids=[p[0] for p in planted_volumes()])
def test_planted_maximum_is_unique_and_decides_g(O, name, ring, make):
    F, at = make()
    mag = M.magnitude(F)
    assert mag[at] == mag.max() and int((mag == mag.max()).sum()) == 1, "the largest magnitude occurs at one voxel only"
    g_rest, g_all = M.g_without(F, at)
    a, b = quantised(ring, g_rest), quantised(ring, g_all)
    inner = (slice(1, -1),) * 3
    changed = int((a[inner] != b[inner]).sum())
    assert 2 * changed > a[inner].size, "a maximum without the planted voxel changes G at %d of %d interior voxels" % (changed, a[inner].size)
    data, _ = M.merge(O, F)                                     # ... and the restatement's G is the one with it
    assert data.dtype == b.dtype and np.array_equal(np.ascontiguousarray(data[..., -1]).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def test_thin_volume_needs_a_second_turn():
    nx, ny, nz = M.THIN
    for ring in M.RINGS:
        tx, ty, tz = M.TILE[ring]
        ux, uy, uz = -(-nx // tx), -(-ny // ty), -(-nz // tz)
        assert ux * uy * uz > M.MAX_BLOCKS
        z, y, x = M.THIN_AT
        assert ((z // tz) * uy + y // ty) * ux + x // tx >= M.MAX_BLOCKS, "the planted voxel's tile is a workgroup's second"


def test_tile_shapes_cover_the_edges():
    for ring in M.RINGS:
        t = M.TILE[ring]
        shapes = M.tile_shapes(ring)
        for a in range(3):
            r = {s[a] % t[a] for s in shapes}
            assert {0, t[a] - 1, 1, 2} <= r, (ring, a, r)
        assert {s[0] & 1 for s in shapes} == {0, 1}
