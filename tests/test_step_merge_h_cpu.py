"""The restatement of the merge with H and blurred normals (tests/_step_merge_h_ref.py) and the volumes of
tests/test_gpu_step_merge_h.py, qualified on the references alone -- the CPU checker's mergeMV, makeVGH and normalsVGH,
_prep_f32_ref -- so that no GPU test can pass vacuously.  No GPU."""
import numpy as np
import pytest

import _prep_f32_ref as P
import _step_merge_h_ref as H
import _step_merge_ref as M


def cases():
    return [(ring, nf, dims) for dims in H.SHAPES for ring in H.RINGS for nf in H.NFS[ring]]


IDS = ["%s-nf%d-%s" % (r, n, "x".join(map(str, d))) for r, n, d in cases()]


# ---- (a) add_h = blur = 0 is the existing merge

@pytest.mark.parametrize("ring, nf", M.CASES)
def test_without_h_and_blur_it_is_the_existing_merge(O, ring, nf):
    F = M.fields(ring, nf, M.SMALL)
    got, want = H.merge_h(F, 0, 1, 0), M.merge(O, F)
    assert got[0].dtype == want[0].dtype and np.array_equal(got[0].view(np.uint8), want[0].view(np.uint8))
    assert np.array_equal(got[1], want[1])
    if ring == "f32":
        f = P.merge_fields_f32(F)
        assert np.array_equal(got[0].view(np.uint32), f[0].view(np.uint32)) and np.array_equal(got[1], f[1])


# ---- (b) H of one u8 field is makeVGH's inside; the border is 85 against makeVGH's 0

@pytest.mark.parametrize("compat", (1, 0))
def test_h_of_one_byte_field_is_make_vghs(O, compat):
    for dims in (M.SMALL, H.MAIN):
        F = H.fields("u8", 1, dims)
        data, _ = H.merge_h(F, 1, compat, 0)
        vgh = O.make_vgh(np.ascontiguousarray(F[..., 0]), compat=bool(compat))
        c = (slice(1, -1),) * 3
        assert np.array_equal(data[c + (2,)], vgh[c + (2,)]), "interior H"
        assert len(np.unique(data[c + (2,)])) > 40
        border = np.ones(data.shape[:3], bool)
        border[c] = False
        assert (data[..., 2][border] == 85).all() and not vgh[..., 2][border].any()
    other = H.merge_h(H.fields("u8", 1, H.MAIN), 1, 1 - compat, 0)[0]
    assert not np.array_equal(other[..., 2], data[..., 2]), "compat decides bytes"


def test_border_h_of_the_float_pipeline():
    data, _ = H.merge_h(H.fields("f32", 2, M.SMALL), 1, 1, 0)
    assert (data[0, :, :, 3] == np.float32(85.0 / 255.0)).all() and (data[:, :, -1, 3] == np.float32(85.0 / 255.0)).all()


# ---- (c) blurred normals of one field are normalsVGH's of a volume whose channel 0 is that field

def test_blurred_normals_of_one_field_are_normals_vghs(O):
    for dims in (M.SMALL, H.MAIN):
        F = H.fields("u8", 1, dims)
        vol = np.ascontiguousarray(np.concatenate([F, F, F], -1))
        for blur in (0, 1):
            nrm = H.merge_h(F, 0, 1, blur)[1]
            assert np.array_equal(nrm, O.normals_vgh(vol, blur=bool(blur))), blur
        assert not np.array_equal(H.merge_h(F, 0, 1, 0)[1], H.merge_h(F, 0, 1, 1)[1])
        Ff = H.fields("f32", 1, dims)
        assert np.array_equal(H.merge_h(Ff, 0, 1, 1)[1], P.normals_f32(Ff, blur=True))
        assert (H.merge_h(F, 0, 1, 1)[1][0] != 128).any(), "a blurred border voxel gathers from the interior"


# ---- (d) the GPU test volumes

@pytest.mark.parametrize("ring, nf, dims", cases(), ids=IDS)
def test_volumes_are_not_vacuous(ring, nf, dims):
    F = H.fields(ring, nf, dims)
    assert F.dtype == H.NP[ring] and F.shape == dims[::-1] + (nf,)
    for compat in (1, 0):
        at, hs = H.extremes_at(F, compat)
        inner = hs[1:-1, 1:-1, 1:-1]
        assert (inner < 0).any() and (inner > 0).any() and np.isnan(inner).any() and np.isnan(hs[1, 1, 1])
        tiles = [H.tile_of(a) for a in at]
        assert all(t != (0, 0, 0) for t in tiles), "an extreme in the first tile: %s" % (tiles,)
        hmin, hmax = H.h_extremes(hs, ring != "u8")
        assert hmin == hs[at[1]] < 0 < hs[at[2]] == hmax
    data, nrm = H.merge_h(F, 1, 1, 1)
    assert np.array_equal(np.ascontiguousarray(data[..., :nf]).view(np.uint8), F.view(np.uint8))
    assert len(np.unique(data[..., nf])) > 60 and len(np.unique(data[..., nf + 1])) > 40
    assert not np.array_equal(nrm, H.merge_h(F, 1, 1, 0)[1])
    # a one-voxel change two voxels across a tile face changes the output voxel: H (and the blurred normal) reach 2
    tx, ty, tz = H.TILE
    for out, src in (((5, 5, tx), (5, 5, tx - 2)), ((5, ty, 7), (5, ty - 2, 7)), ((tz, 5, 7), (tz - 2, 5, 7)),
                     ((5, 5, tx - 1), (5, 5, tx + 1)), ((5, ty - 1, 7), (5, ty + 1, 7)), ((tz - 1, 5, 7), (tz + 1, 5, 7))):
        assert H.tile_of(out) != H.tile_of(src)
        G = F.copy()
        G[src] = 0 if F[src + (0,)] > F.max() / 2 else F.max()
        for add_h, blur in ((1, 0), (0, 1)):
            # (compat 0: the reference's typo drops h[4], the one term through which H sees two voxels along y)
            a, b = H.merge_h(F, add_h, 0, blur), H.merge_h(G, add_h, 0, blur)
            ch = a[0][out][nf + 1:] if add_h else a[1][out]
            ch2 = b[0][out][nf + 1:] if add_h else b[1][out]
            assert not np.array_equal(ch, ch2), "the voxel %s does not see %s (add_h %d, blur %d)" % (out, src, add_h, blur)
            if not add_h:                                   # (the plain merge reaches 1: G and plain normals do not see it)
                p, q = H.merge_h(F, 0, 1, 0), H.merge_h(G, 0, 1, 0)
                assert np.array_equal(p[1][out], q[1][out])


@pytest.mark.parametrize("ring", H.RINGS)
def test_thin_volume_needs_a_second_turn(ring):
    nx, ny, nz = H.THIN
    tx, ty, tz = H.TILE
    gx, gy, gz = -(-nx // tx), -(-ny // ty), -(-nz // tz)
    assert gx * gy * gz > H.STATS_BLOCKS
    F = H.thin_fields(ring)
    at, hs = H.extremes_at(F)
    for z, y, x in at:
        assert ((z // tz) * gy + y // ty) * gx + x // tx >= H.STATS_BLOCKS, "an extreme's tile is a workgroup's first"
    # ... and each decides stored values: without the last layer of tiles the extremes differ
    cut = np.ascontiguousarray(F[:(H.THIN_AT[0] // tz) * tz])
    at2, hs2 = H.extremes_at(cut)
    flt = ring != "u8"
    assert H.h_extremes(hs, flt)[0] != H.h_extremes(hs2, flt)[0] and H.h_extremes(hs, flt)[1] != H.h_extremes(hs2, flt)[1]


def test_degenerate_inputs():
    flat = np.full((6, 5, 7, 2), 93, np.uint8)
    data, nrm = H.merge_h(flat, 1, 1, 1)
    assert not data[..., 2].any() and (nrm == 128).all()
    assert not data[1:-1, 1:-1, 1:-1, 3].any() and (data[0, ..., 3] == 85).all()      # every interior H NaN -> 0; the border 85
    dataf, _ = H.merge_h(flat.astype(np.float32), 1, 1, 0)
    assert not dataf[1:-1, 1:-1, 1:-1, 3].any() and (dataf[0, ..., 3] == np.float32(85.0 / 255.0)).all()


def test_shapes_cover_the_tile_edges():
    for a in range(3):
        assert {s[a] % H.TILE[a] for s in H.SHAPES} >= {H.TILE[a] - 1, 0, 1, 2, 3}
        assert all(s[a] > H.TILE[a] for s in H.SHAPES)
    assert {s[0] & 1 for s in H.SHAPES} == {0, 1}
