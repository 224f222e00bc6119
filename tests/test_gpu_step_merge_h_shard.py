"""The merge with H and blurred normals on sharded contexts and from blocks (smk.h: smk_step_extremes_h_device,
smk_merge_timestep_h_shard, smk_block_extremes_h_device, smk_upload_timestep_fields_h_block_device).  Expected voxels come
from the EXISTING one-call entries, smk_merge_timestep_h and smk_upload_timestep_fields_h_device, run in the same test on an
unsharded context that holds the whole volume: the ranks' words, regions, halo voxels, histograms and frames must be that
context's.  The cases are tests/_step_merge_h_shard_ref.py's (qualified by tests/test_step_merge_h_shard_cpu.py): volumes of
a few ten thousand voxels."""
import ctypes

import numpy as np
import pytest

import _step_block_ref as B
import _step_merge_h_ref as H
import _step_merge_h_shard_ref as R
import _step_shard_ref as S
import _tblend_ref as T
from _gpu_mem import dev_ptr as dev, merged, words_buf
from _step_gpu import (RAN, SORT_LAST_TOL, UndisturbedHalos, close, declared, flags_of, fsz, probe_at, rank_context, ranks_declared,
                       ranks_of, run_cut, same_bits as same)

pytestmark = pytest.mark.gpu
CODE = H.CODE
REACH = R.REACH


def mode(nelts, add_h):
    return H.MODE[(nelts - 1 - add_h, add_h)]


def export(C, src, add_h, compat, stream=None):
    import torch
    w = words_buf()
    C.step_extremes_h_device(src, w.data_ptr(), add_h=add_h, compat=compat, stream=stream)
    torch.cuda.synchronize()                                # the export ran on the context's stream, or the caller's: read-back
    return w.cpu().numpy()[0]


_REF = {}


def reference(factory, case, ring, nf, add_h, blur, compat, normals=True):
    """what smk_merge_timestep_h makes of the case's source on an unsharded context, made once and shared: (source data, source
    normals, result data, result normals, probe(cells) of the result, its hist2d_step counts)"""
    key = (case, ring, nf, add_h, blur, compat, normals)
    if key not in _REF:
        dims = R.CASES[case][0]
        data, grad = R.source(case, ring, nf, add_h)
        grad = grad if normals else None
        U = rank_context(factory, dims, data, grad, mode(data.shape[-1], add_h))
        try:
            U.merge_timestep_h(0, 1, add_h, compat, blur)
            got = U.download_timestep(1)
            probe = U.probe_step(S.cells_of((0, 0, 0), dims), 1)
            hist = U.hist2d_step(1)
            assert probe[2].all() and got[0][..., nf].any()
        finally:
            U.close()
        for a in got + probe[:2]:
            a.setflags(write=False)
        _REF[key] = (data, grad, got[0], got[1], probe, hist)
    return _REF[key]


CASES = [pytest.param(i, ring, id="%s-%s" % (R.CASE_IDS[i], ring)) for i in range(len(R.CASES)) for ring in R.RINGS]


# ---- 1. the words

@pytest.mark.parametrize("case, ring", CASES)
def test_the_ranks_words_combine_to_the_unsharded_words(gpu_renderer_factory, case, ring):
    dims, nranks, halo = R.CASES[case]
    seen = set()
    for nf, add_h, blur, compat in R.layouts(case, ring):
        if (nf, add_h, compat) in seen:                     # (blur is no matter of pass 1)
            continue
        seen.add((nf, add_h, compat))
        data, grad = R.source(case, ring, nf, add_h)
        U = rank_context(gpu_renderer_factory, dims, data, grad, mode(data.shape[-1], add_h))
        try:
            want = export(U, 0, add_h, compat)
        finally:
            U.close()
        rs = ranks_of(gpu_renderer_factory, dims, data, grad, mode(data.shape[-1], add_h), nranks, halo)
        try:
            words = [export(C, 0, add_h, compat) for C in rs]
        finally:
            close(rs)
        what = (nf, add_h, compat)
        assert np.array_equal(R.combine(words), want), (what, words, want)
        assert (want[3:] == R.INT_MIN).all() and want[0] > 0, what
        assert (not np.array_equal(want[1:3], R.WORD_SEEDS[1:3])) == bool(add_h), what
        F = R.fields(case, ring, nf)
        for r, w in enumerate(words):
            g0, g1 = R.stored_box(dims, r, nranks, halo, ring)[:2]
            assert np.array_equal(w, R.region_words(F, g0, g1, add_h, compat)), "%s rank %d: %s, the restatement has %s" % (
                what, r, w, R.region_words(F, g0, g1, add_h, compat))
            assert np.array_equal(w, R.WORD_SEEDS) == (not S.has_interior(dims, g0, g1)), (what, r)


# ---- 2. the two-call form on an unsharded context

TWO_CALL = [("u8", 2, 1, 1), ("u8", 2, 1, 2), ("u16", 1, 1, 1), ("u16", 1, 1, 2), ("f32", 1, 1, 1), ("f32", 1, 1, 2), ("u8", 3, 0, 2), ("u16", 2, 0, 1),
            ("f32", 2, 1, 1), ("f32", 3, 0, 1)]                # (four-channel f32 voxels: the gather kernel alone renders them)


@pytest.mark.parametrize("ring, nf, add_h, kernel", TWO_CALL)
def test_export_and_write_on_an_unsharded_context_is_the_one_call_entry(gpu_renderer_factory, smk, ring, nf, add_h, kernel):
    """both source forms: a resident step, and dense fields handed over as a whole-volume block"""
    import torch
    from _scenes import push_scene
    dims = (37, 13, 11)                                     # (odd x and y: a pad column and row of 8-byte voxels)
    F = H.fields(ring, nf, dims, 0)
    data, grad = H.source_step(F, add_h)
    sc = T.scene(np.ascontiguousarray(data[..., :3]), grad)
    held = [dev(np.ascontiguousarray(F[..., e])) for e in range(nf)]
    ptrs = [h[0] for h in held]
    C = rank_context(gpu_renderer_factory, dims, data, grad, mode(data.shape[-1], add_h), cap=6, opts=(("kernel", kernel),))
    try:
        push_scene(C, sc, upload=False)
        C.merge_timestep_h(0, 1, add_h, 1, 1)
        C.upload_timestep_fields_h_device(4, ptrs, CODE[ring], dims, add_h, 1, 1)
        w = words_buf(2)
        C.step_extremes_h_device(0, w[0].data_ptr(), add_h=add_h)
        C.merge_timestep_h_shard(0, 2, w[0].data_ptr(), add_h=add_h, blur=1)
        blk = smk.smk_block((0, 0, 0), dims)
        C.block_extremes_h_device(ptrs, CODE[ring], blk, w[1].data_ptr(), add_h=add_h)
        C.upload_timestep_fields_h_block_device(3, ptrs, CODE[ring], blk, w[1].data_ptr(), add_h=add_h, blur=1)
        assert [C.timestep_halo(t) for t in range(5)] == [1] * 5
        torch.cuda.synchronize()                            # (the exports ran on the context's stream)
        ws = w.cpu().numpy()
        assert np.array_equal(ws[0], ws[1]) and np.array_equal(ws[0], R.region_words(F, (0, 0, 0), dims, add_h, 1))
        a, a2 = C.download_timestep(1), C.download_timestep(4)
        same(a2[0], a[0], "the two one-call entries: data")
        assert not np.array_equal(a[0], C.download_timestep(0)[0]) and (a[1] != 128).any()
        for t, what in ((2, "a resident step"), (3, "a whole-volume block")):
            b = C.download_timestep(t)
            same(b[0], a[0], what + ": data")
            same(b[1], a[1], what + ": normals")            # (nelts 4 in an f32 ring: the separate normals buffer)
        frames = []
        for t in (1, 2, 3):
            C.select_timestep(t)
            frames.append(C.render())
            assert C.last_frame_info()[0] == RAN[kernel]
        assert C.stat("slab_failures") == 0
    finally:
        C.close()
    del held
    assert frames[0][..., 3].max() > 0.05
    assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])


# ---- 3. the regions, the halo, the rim, the probe and the histogram on 2, 4 and 8 ranks

def check_ranks(factory, case, ring, nf, add_h, blur, compat, normals=True):
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = R.CASES[case]
    data, grad, wdata, wgrad, wprobe, whist = reference(factory, case, ring, nf, add_h, blur, compat, normals)
    what = "nf %d add_h %d blur %d compat %d" % (nf, add_h, blur, compat)
    rs = ranks_of(factory, dims, data, grad, mode(data.shape[-1], add_h), nranks, halo)
    try:
        sortlast.stencil_timestep_local(rs, "merge_h", 0, 1, compat=compat, blur=blur, add_h=add_h)
        parts, gparts, hist, rim_seen = [], [], np.zeros((256, 256), np.int64), False
        for r, C in enumerate(rs):
            g0, g1, O, Dd, pad = R.stored_box(dims, r, nranks, halo, ring)
            origin, size, ne, dt, hn = C.timestep_box()
            assert origin == g0 and size == tuple(b - a for a, b in zip(g0, g1)) and hn == normals
            got = C.download_timestep(1)
            parts.append((origin, got[0]))
            gparts.append((origin, got[1]))
            assert C.timestep_halo(0) == halo and C.timestep_halo(1) == halo - REACH, what
            assert C.timesteps() == (0, [0, 1])
            hist += C.hist2d_step(1)
            # every cell of the stored box that lies in the volume: answered inside the valid box, and only there
            lo, hi = R.valid_box(dims, O, Dd, REACH)
            slo, shi = S.uploaded_valid(dims, O, Dd)
            rim_seen |= (lo, hi) != (slo, shi)
            cells = S.cells_of(slo, shi)
            raw, nrm, ok = C.probe_step(cells, 1)
            inside = np.all((cells >= np.array(lo)) & (cells + 1 < np.array(hi)), -1)
            assert np.array_equal(ok, inside), "%s rank %d: %d cells answered, %d lie in the valid box" % (what, r, ok.sum(), inside.sum())
            assert (S.straddles(cells, g0, g1) & inside).any(), "a cell with a corner in the halo"
            wraw, wnrm = probe_at(wprobe, dims, cells[inside])
            same(raw[inside], wraw, "%s rank %d: the valid box's voxels" % (what, r))
            same(nrm[inside], wnrm, "%s rank %d: the valid box's normals" % (what, r))
            assert not raw[~inside].any() and not nrm[~inside].any()
        assert rim_seen == (dims[0] != 3)                   # (3 voxels thick: every rank stores the whole volume)
    finally:
        close(rs)
    same(S.place(dims, wdata.shape[-1], wdata.dtype, parts), wdata, what + ": data")
    same(S.place(dims, 3, np.uint8, gparts), wgrad, what + ": normals")
    assert np.array_equal(hist, whist.astype(np.int64)), what + ": the ranks' histogram counts sum to the unsharded counts"
    if not normals:
        assert (wgrad == 128).all()


@pytest.mark.parametrize("case, ring", CASES)
def test_the_ranks_regions_and_halos_are_the_unsharded_step(gpu_renderer_factory, case, ring):
    for nf, add_h, blur, compat in R.layouts(case, ring):
        check_ranks(gpu_renderer_factory, case, ring, nf, add_h, blur, compat)


@pytest.mark.parametrize("ring, nf, add_h", [("u8", 2, 1), ("u16", 1, 1), ("f32", 2, 1), ("f32", 2, 0)])
def test_the_rim_is_zeros_with_normal_128(gpu_renderer_factory, ring, nf, add_h):
    """Nothing reads a stored voxel outside a step's valid box back; the brick summaries are made over the whole stored box,
    and the brick flags show them.  A step of top values is overwritten in place by the write pass: under a table that is
    opaque at the top values alone the flags must be those of a context that UPLOADED the result with its rim zeroed, and
    differ from those of one that uploaded it with the top values left on the rim."""
    case, blur, compat = 0, 1, 1
    dims, nranks, halo = R.CASES[case]
    data, grad, wdata, wgrad, _, _ = reference(gpu_renderer_factory, case, ring, nf, add_h, blur, compat)
    ne = data.shape[-1]
    top = {"u8": 255, "u16": 65535, "f32": 1.0}[ring]
    stale = np.full(data.shape, top, data.dtype)
    sgrad = np.full(grad.shape, 7, np.uint8)
    sc = T.scene(np.ascontiguousarray(wdata[..., :3]), wgrad)
    table = np.zeros((256, 256, 4), np.uint8)
    table[250:, 250:] = 255
    opts = (("kernel", 1),)
    told = False
    for r in range(nranks):
        g0, g1, O, Dd, pad = R.stored_box(dims, r, nranks, halo, ring)
        lo, hi = R.valid_box(dims, O, Dd, REACH)
        outside = ~S.in_box(dims[::-1], (0, 0, 0), lo, hi)
        want = []
        for fill, gfill in ((0, 128), (top, 7)):
            d, g = wdata.copy(), wgrad.copy()
            d[outside], g[outside] = fill, gfill
            U = rank_context(gpu_renderer_factory, dims, d, g, mode(d.shape[-1], add_h), r, nranks, halo, opts=opts)
            try:
                want.append(flags_of(U, sc, 0, [table])[0])
            finally:
                U.close()
        C = rank_context(gpu_renderer_factory, dims, data, grad, mode(ne, add_h), r, nranks, halo, cap=3, opts=opts)
        try:
            import torch
            C.upload_timestep(1, stale, sgrad, fsize=fsz(dims), dmode=mode(ne, add_h))
            before = flags_of(C, sc, 1, [table])[0]
            w = words_buf()
            wu = export_unsharded(gpu_renderer_factory, case, ring, nf, add_h, compat)
            w[0] = torch.tensor(wu, dtype=torch.int32)
            torch.cuda.synchronize()                        # the words are on the device before the context's stream reads them
            C.merge_timestep_h_shard(0, 1, w.data_ptr(), add_h=add_h, compat=compat, blur=blur)
            assert C.timesteps() == (1, [0, 1]) and C.timestep_halo(1) == halo - REACH     # (the shown step, overwritten in place)
            got = flags_of(C, sc, 1, [table])[0]
        finally:
            C.close()
        assert before.all(), "the stale step flags every brick"
        assert np.array_equal(got, want[0]), "rank %d: %d bricks differ from the zeroed rim's" % (r, (got != want[0]).sum())
        told |= not np.array_equal(want[1], want[0])
    assert told, "the table tells a stale rim from a zeroed one on some rank"


_WORDS = {}


def export_unsharded(factory, case, ring, nf, add_h, compat):
    key = (case, ring, nf, add_h, compat)
    if key not in _WORDS:
        data, grad = R.source(case, ring, nf, add_h)
        U = rank_context(factory, R.CASES[case][0], data, grad, mode(data.shape[-1], add_h))
        try:
            _WORDS[key] = export(U, 0, add_h, compat)
        finally:
            U.close()
    return _WORDS[key]


# ---- 4. the block form

def block_reference(factory, case, ring, nf, add_h, blur, compat, normals=True):
    """what smk_upload_timestep_fields_h_device makes of the whole dense fields on an unsharded context: (the arrays, result
    data, result normals, probe(cells))"""
    key = ("block", case, ring, nf, add_h, blur, compat, normals)
    if key not in _REF:
        dims = R.CASES[case][0]
        F = R.fields(case, ring, nf)
        arr = [np.ascontiguousarray(F[..., e]) for e in range(nf)]
        held = [dev(a) for a in arr]
        U = declared(factory, dims, ring, nf + 1 + add_h, mode(nf + 1 + add_h, add_h), normals=normals)
        try:
            U.upload_timestep_fields_h_device(1, [h[0] for h in held], CODE[ring], dims, add_h, compat, blur)
            got = U.download_timestep(1)
            probe = U.probe_step(S.cells_of((0, 0, 0), dims), 1)
            assert probe[2].all() and got[0][..., nf].any()
        finally:
            U.close()
        del held
        _REF[key] = (arr, got[0], got[1], probe)
    return _REF[key]


def cuts_of(case, ring, which):
    dims, nranks, halo = R.CASES[case]
    return [B.Cut("derive", dims, r, nranks, halo, ring, which, reach=REACH) for r in range(nranks)]


def check_blocks(factory, smk, case, ring, nf, add_h, blur, compat, normals=True, which=B.CUTS):
    dims, nranks, halo = R.CASES[case]
    arr, wdata, wgrad, wprobe = block_reference(factory, case, ring, nf, add_h, blur, compat, normals)
    wwords = export_unsharded(factory, case, ring, nf, add_h, compat)
    F = R.fields(case, ring, nf)
    for group in (("a", "b"), ("c",)):                      # (a) and (b) share option halo, and so their contexts
        group = [wc for wc in group if wc in which]
        if not group:
            continue
        all_cuts = [cuts_of(case, ring, wc) for wc in group]
        rs = ranks_declared(factory, dims, ring, nf + 1 + add_h, mode(nf + 1 + add_h, add_h), all_cuts[0], normals)
        try:
            for out, cuts in enumerate(all_cuts, 1):
                keep, words = run_cut(smk, rs, cuts, "merge_h", ring, ring, arr, out, compat, blur, add_h=add_h)
                w = words.cpu().numpy()
                assert np.array_equal(w[nranks], wwords), (w, wwords)
                parts, gparts = [], []
                for C, c in zip(rs, cuts):
                    what = "cut %s rank %d" % (c.which, c.rank)
                    assert np.array_equal(w[c.rank], R.region_words(F, c.g0, c.g1, add_h, compat)), what
                    if c.which == "c" and case < 3:         # (the small volumes: C reaches the volume's faces, which give all a halo can)
                        assert c.src_halo == REACH + 1, "ghost cells of exactly 3"
                    got = C.download_timestep(out)
                    parts.append((c.g0, got[0]))
                    gparts.append((c.g0, got[1]))
                    assert C.timestep_halo(out) == c.halo == c.src_halo - REACH, what
                    cells = S.cells_of(c.stored_lo, c.stored_hi)
                    raw, nrm, ok = C.probe_step(cells, out)
                    inside = np.all((cells >= np.array(c.vlo)) & (cells + 1 < np.array(c.vhi)), -1)
                    assert np.array_equal(ok, inside), "%s: %d cells answered, %d lie in the valid box" % (what, ok.sum(), inside.sum())
                    assert (S.straddles(cells, c.g0, c.g1) & inside).any()
                    wraw, wnrm = probe_at(wprobe, dims, cells[inside])
                    same(raw[inside], wraw, what + ": the valid box's voxels")
                    same(nrm[inside], wnrm, what + ": the valid box's normals")
                same(S.place(dims, wdata.shape[-1], wdata.dtype, parts), wdata, "data")
                same(S.place(dims, 3, np.uint8, gparts), wgrad, "normals")
                del keep
        finally:
            close(rs)


@pytest.mark.parametrize("case, ring", CASES)
def test_the_ranks_blocks_give_the_unsharded_step(gpu_renderer_factory, smk, case, ring):
    """cut (a): region +- option halo; (b): a pitched view of the whole arrays with poison outside it, ending on the volume's
    face where the stored box does; (c): ghost cells of exactly 3 under a larger option halo"""
    for nf, add_h, blur, compat in R.layouts(case, ring):
        if case == 0 and (blur, compat) != (1, 1):          # (the flags' other values: the resident form above)
            continue
        check_blocks(gpu_renderer_factory, smk, case, ring, nf, add_h, blur, compat)


# ---- 5. a context without normals

@pytest.mark.parametrize("ring, nf, add_h", [("u8", 2, 1), ("u16", 2, 0), ("f32", 2, 1), ("f32", 1, 1)])
def test_a_context_without_normals(gpu_renderer_factory, smk, ring, nf, add_h):
    check_ranks(gpu_renderer_factory, 0, ring, nf, add_h, 1, 1, normals=False)
    check_blocks(gpu_renderer_factory, smk, 0, ring, nf, add_h, 1, 1, normals=False, which=("a",))


# ---- 6. frames

@pytest.mark.parametrize("kernel", [1, 2], ids=["gather", "slice-ring"])
@pytest.mark.parametrize("case, ring, nf, add_h", [(0, "u8", 2, 1), (2, "u16", 1, 1), (0, "f32", 1, 1), (2, "f32", 2, 0)])
def test_frames_of_the_produced_step(gpu_renderer_factory, case, ring, nf, add_h, kernel):
    from _scenes import push_scene
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = R.CASES[case]
    data, grad, wdata, wgrad, _, _ = reference(gpu_renderer_factory, case, ring, nf, add_h, 1, 1)
    opts = (("kernel", kernel), ("slab_split", 1))
    sc = T.scene(np.ascontiguousarray(wdata[..., :3]), wgrad)

    def frames(rs):
        for C in rs:
            push_scene(C, sc, upload=False)
        lay, out = merged(rs, sc)
        assert all(C.last_frame_info()[0] == RAN[kernel] for C in rs) and all(C.stat("slab_failures") == 0 for C in rs)
        return lay, out
    U = rank_context(gpu_renderer_factory, dims, wdata, wgrad, mode(wdata.shape[-1], add_h), opts=opts)
    try:
        push_scene(U, sc, upload=False)
        whole = U.render()
    finally:
        U.close()
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, mode(data.shape[-1], add_h), nranks, halo, opts=opts)
    try:
        frames(rs)                                          # (the source rendered first: flags and plans of another step exist)
        keep = sortlast.stencil_timestep_local(rs, "merge_h", 0, 1, compat=1, blur=1, add_h=add_h)
        for C in rs:
            C.select_timestep(1)
        got_layers, got = frames(rs)
        del keep
    finally:
        close(rs)
    assert whole[..., 3].max() > 0.05 and all(l[..., 3].max() > 0.01 for l in got_layers)
    err = np.abs(got - whole).max()
    assert err <= SORT_LAST_TOL, "merged against the unsharded frame: max abs err %g" % err


# ---- 7. a chain

@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("ring", ["u8", "f32"])
def test_a_chain_of_stencils(gpu_renderer_factory, smk, ring, nranks):
    """upload at halo 5 -> merge_h (nelts 3, V1GH) leaving halo 3 -> derive of its channel 0 leaving halo 1 -> a third stencil
    refused; and a blend of two uploads feeding merge_h.  Every step against the same chain on an unsharded context, inside
    the valid box the steps shrink to"""
    from simian_spacemonkey_amd import sortlast
    dims, halo = (45, 21, 19), 5
    F0, F1 = H.fields(ring, 1, dims, 0), H.fields(ring, 1, dims, 1)
    (d0, g0), (d1, g1) = H.source_step(F0, 1), H.source_step(F1, 1, seed=6)
    cells = S.cells_of((0, 0, 0), dims)
    U = rank_context(gpu_renderer_factory, dims, d0, g0, "V1GH", cap=6)
    try:
        U.upload_timestep(1, d1, g1, fsize=fsz(dims), dmode="V1GH")
        U.merge_timestep_h(0, 2, 1, 1, 1)
        U.derive_timestep(2, 3, 1, 1)
        U.blend_timesteps(0, 1, 0.37, 4)
        U.merge_timestep_h(4, 5, 1, 0, 0)
        want = {t: U.probe_step(cells, t) for t in (2, 3, 4, 5)}
    finally:
        U.close()
    rs = ranks_of(gpu_renderer_factory, dims, d0, g0, "V1GH", nranks, halo, cap=6)
    try:
        for C in rs:
            C.upload_timestep(1, d1, g1, fsize=fsz(dims), dmode="V1GH")
        keep = [sortlast.stencil_timestep_local(rs, "merge_h", 0, 2, compat=1, blur=1, add_h=1)]
        keep.append(sortlast.stencil_timestep_local(rs, "derive", 2, 3, compat=1, blur=1))
        for C in rs:
            C.blend_timesteps(0, 1, 0.37, 4)
        keep.append(sortlast.stencil_timestep_local(rs, "merge_h", 4, 5, compat=0, blur=0, add_h=1))
        for r, C in enumerate(rs):
            g0r, g1r, O, Dd, pad = R.stored_box(dims, r, nranks, halo, ring)
            up = S.uploaded_valid(dims, O, Dd)
            once = S.valid_box(dims, O, Dd, 2, src=up)
            twice = S.valid_box(dims, O, Dd, 2, src=once)
            assert [C.timestep_halo(t) for t in range(6)] == [5, 5, 3, 1, 5, 3]
            for t, (lo, hi) in ((2, once), (3, twice), (4, up), (5, once)):
                cs = S.cells_of(*up)
                raw, nrm, ok = C.probe_step(cs, t)
                inside = np.all((cs >= np.array(lo)) & (cs + 1 < np.array(hi)), -1)
                assert np.array_equal(ok, inside), "rank %d step %d: %d cells answered, %d lie in the valid box" % (r, t, ok.sum(), inside.sum())
                wraw, wnrm = probe_at(want[t], dims, cs[inside])
                same(raw[inside], wraw, "rank %d step %d: voxels" % (r, t))
                same(nrm[inside], wnrm, "rank %d step %d: normals" % (r, t))
            before = C.timesteps()
            w = words_buf()
            for call in (lambda: C.step_extremes_h_device(3, w.data_ptr()), lambda: C.merge_timestep_h_shard(3, 0, w.data_ptr()),
                         lambda: C.derive_timestep_shard(3, 0, w.data_ptr())):
                with pytest.raises(smk.SmkError, match=r"time step 3 \(the source\) has a valid halo of 1 voxels, the stencil reaches 2 .*>= 3 is needed"):
                    call()
            assert C.timesteps() == before
        del keep
    finally:
        close(rs)


# ---- 8. streams, and a cached output that is the current step

def test_on_a_stream_of_the_callers_and_in_place(gpu_renderer_factory):
    """export, combine and write on a non-default stream with no host wait, then an upload over the source on another stream;
    then the same output id again while it is the step the frames render.  The bits are those of the contexts' own streams"""
    import torch
    from _scenes import push_scene
    from simian_spacemonkey_amd import sortlast
    case, ring, nf, add_h = 0, "u8", 2, 1
    dims, nranks, halo = R.CASES[case]
    data, grad, wdata, wgrad, _, _ = reference(gpu_renderer_factory, case, ring, nf, add_h, 1, 1)
    data2, grad2 = H.source_step(H.fields(ring, nf, dims, 1), add_h, seed=6)
    sc = T.scene(np.ascontiguousarray(wdata[..., :3]), wgrad)

    def run(side, other):
        rs = ranks_of(gpu_renderer_factory, dims, data, grad, mode(data.shape[-1], add_h), nranks, halo, opts=(("kernel", 1),))
        try:
            for C in rs:
                push_scene(C, sc, upload=False)
            pd, k0 = dev(data2)
            pg, k1 = dev(grad2)
            st = None if side is None else ctypes.c_void_p(side.cuda_stream)
            keep = [sortlast.stencil_timestep_local(rs, "merge_h", 0, 1, compat=1, blur=1, stream=st, add_h=add_h)]
            for C in rs:                                    # the source slot overwritten: behind the write pass's reads
                C.upload_timestep_device(0, pd, dims, data2.shape[-1], CODE[ring], pg, fsize=fsz(dims), dmode=mode(data2.shape[-1], add_h),
                                         stream=None if other is None else ctypes.c_void_p(other.cuda_stream))
                C.select_timestep(1)
            lay, out = merged(rs, sc)
            downs = [C.download_timestep(1) for C in rs]
            # in place: step 1 is current and cached; made again from the new step 0, it stays current
            keep.append(sortlast.stencil_timestep_local(rs, "merge_h", 0, 1, compat=1, blur=1, stream=st, add_h=add_h))
            assert all(C.timesteps() == (1, [0, 1]) for C in rs)
            lay2, out2 = merged(rs, sc)
            downs += [C.download_timestep(1) for C in rs]
            del keep, k0, k1
            return lay, out, downs, out2
        finally:
            close(rs)
    want = run(None, None)
    got = run(torch.cuda.Stream(), torch.cuda.Stream())
    assert want[1][..., 3].max() > 0.05 and not np.array_equal(want[1], want[3])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[3], want[3])
    for (a, b), (c, d) in zip(want[2], got[2]):
        same(c, a, "a step made on the caller's stream")
        same(d, b, "its normals")
    g0r, g1r = R.stored_box(dims, 0, nranks, halo, ring)[:2]
    same(got[2][0][0], wdata[g0r[2]:g1r[2], g0r[1]:g1r[1], g0r[0]:g1r[0]], "rank 0's region")
    U = rank_context(gpu_renderer_factory, dims, data2, grad2, mode(data2.shape[-1], add_h))
    try:
        U.merge_timestep_h(0, 1, add_h, 1, 1)
        again = U.download_timestep(1)[0]
    finally:
        U.close()
    same(got[2][nranks][0], again[g0r[2]:g1r[2], g0r[1]:g1r[1], g0r[0]:g1r[0]], "rank 0's region, made again in place")


# ---- 9. refusals

def test_refusals_leave_the_ring_unchanged(gpu_renderer_factory, smk):
    from _scenes import push_scene
    dims, nranks, ring = (37, 13, 11), 2, "u8"
    F = H.fields(ring, 2, dims, 0)
    data, grad = H.source_step(F, 1)
    sc = T.scene(np.ascontiguousarray(data[..., :3]), grad)
    held = [dev(np.ascontiguousarray(F[..., e])) for e in range(2)]
    ptrs = [h[0] for h in held]
    w = words_buf()
    p = w.data_ptr()
    whole = smk.smk_block((0, 0, 0), dims)
    entries = ("smk_step_extremes_h_device", "smk_merge_timestep_h_shard", "smk_block_extremes_h_device", "smk_upload_timestep_fields_h_block_device")
    C = gpu_renderer_factory()
    try:
        for call, who in ((lambda: C.step_extremes_h_device(0, p), entries[0]), (lambda: C.merge_timestep_h_shard(0, 1, p), entries[1]),
                          (lambda: C.block_extremes_h_device(ptrs, 0, whole, p), entries[2]),
                          (lambda: C.upload_timestep_fields_h_block_device(1, ptrs, 0, whole, p), entries[3])):
            with pytest.raises(smk.SmkError, match=who + ": no volume"):
                call()
    finally:
        C.close()
    # a ring of two slots, both held: the source and the current step leave no slot for the output
    g0, g1, O, Dd, pad = R.stored_box(dims, 0, nranks, REACH + 1, ring)
    C = rank_context(gpu_renderer_factory, dims, data, grad, "V2GH", 0, nranks, REACH + 1, cap=2, opts=(("kernel", 1),))
    try:
        push_scene(C, sc, upload=False)
        C.upload_timestep(1, data, grad, fsize=fsz(dims), dmode="V2GH")
        short = smk.smk_block((0, 0, 0), (g1[0] + REACH, dims[1], dims[2]))        # a valid halo of 2
        miss = smk.smk_block((0, 0, 0), (g1[0] - 1, dims[1], dims[2]))             # C misses the region's last column
        with UndisturbedHalos(C, downloads=False):
            for call, why in (
                    (lambda: C.step_extremes_h_device(0, p, add_h=2), "smk_step_extremes_h_device: add_h 2 is neither 0 nor 1"),
                    (lambda: C.merge_timestep_h_shard(1, 5, p, add_h=-1), "smk_merge_timestep_h_shard: add_h -1 is neither 0 nor 1"),
                    (lambda: C.merge_timestep_h_shard(1, 5, p, blur=2), "smk_merge_timestep_h_shard: blur 2 is neither 0 nor 1"),
                    (lambda: C.block_extremes_h_device(ptrs, 0, whole, p, add_h=3), "smk_block_extremes_h_device: add_h 3 is neither"),
                    (lambda: C.upload_timestep_fields_h_block_device(5, ptrs, 0, whole, p, blur=-1), "fields_h_block_device: blur -1 is neither"),
                    (lambda: C.merge_timestep_h_shard(99, 5, p), r"smk_merge_timestep_h_shard: time step 99 \(the source\) is not cached"),
                    (lambda: C.step_extremes_h_device(99, p), r"smk_step_extremes_h_device: time step 99 \(the source\) is not cached"),
                    (lambda: C.merge_timestep_h_shard(0, -1, p), "ids are >= 0"),
                    (lambda: C.merge_timestep_h_shard(1, 1, p), "output time step 1 is also the source: the stencil has no in-place form"),
                    (lambda: C.merge_timestep_h_shard(1, 5, p), r"smk_merge_timestep_h_shard: the cache holds 2 steps.*here 3"),
                    (lambda: C.merge_timestep_h_shard(1, 5, None), "d_words is NULL"),
                    (lambda: C.merge_timestep_h_shard(1, 5, p + 2), "d_words is not aligned to its 4-byte words"),
                    (lambda: C.step_extremes_h_device(0, None), "smk_step_extremes_h_device: d_words is NULL"),
                    (lambda: C.step_extremes_h_device(0, p + 1), "d_words is not aligned"),
                    (lambda: C.block_extremes_h_device(ptrs, 0, whole, None), "smk_block_extremes_h_device: d_words is NULL"),
                    (lambda: C.upload_timestep_fields_h_block_device(1, ptrs, 0, whole, p + 2), "d_words is not aligned"),
                    (lambda: C.block_extremes_h_device(ptrs, 0, miss, p), r"holds voxels \[0, %d\) of axis x .* its region is \[0, %d\)" % (g1[0] - 1, g1[0])),
                    (lambda: C.upload_timestep_fields_h_block_device(1, ptrs, 0, miss, p), "the block must contain the region"),
                    (lambda: C.block_extremes_h_device(ptrs, 0, short, p), r"the block gives a valid halo of 2 voxels, the stencil reaches 2 .*>= 3 is needed"),
                    (lambda: C.upload_timestep_fields_h_block_device(1, ptrs, 0, short, p), r"valid halo of 2 voxels, the stencil reaches 2 .*>= 3"),
                    (lambda: C.block_extremes_h_device(ptrs[:1], 0, whole, p), "1 fields for a series of nelts 4 with add_h 1: the fields are nelts - 1 - add_h = 2"),
                    (lambda: C.block_extremes_h_device(ptrs, 0, whole, p, add_h=0), "2 fields for a series of nelts 4 with add_h 0"),
                    (lambda: C.upload_timestep_fields_h_block_device(1, ptrs + ptrs[:1], 0, whole, p), "3 fields for a series of nelts 4"),
                    (lambda: C.block_extremes_h_device(ptrs, 1, whole, p), r"field_dtype 1 is not the ring's type \(0\)"),
                    (lambda: C.upload_timestep_fields_h_block_device(1, ptrs, 2, whole, p), "field_dtype 2 is not the ring's type"),
                    (lambda: C.block_extremes_h_device(None, 0, whole, p), "d_fields is NULL"),
                    (lambda: C.block_extremes_h_device([ptrs[0], None], 0, whole, p), r"d_fields\[1\] is NULL"),
                    (lambda: C.block_extremes_h_device(ptrs, 0, None, p), "block is NULL")):
                with pytest.raises(smk.SmkError, match=why):
                    call()
        assert (w.cpu().numpy() == 0x5a5a5a5a).all(), "a refused export writes no word"
    finally:
        C.close()
    # the source's valid halo below reach + 1: the message names 2 and 3
    C = rank_context(gpu_renderer_factory, dims, data, grad, "V2GH", 0, nranks, 2, cap=3, opts=(("kernel", 1),))
    try:
        push_scene(C, sc, upload=False)
        with UndisturbedHalos(C, downloads=False):
            for call in (lambda: C.merge_timestep_h_shard(0, 1, p), lambda: C.step_extremes_h_device(0, p),
                         lambda: C.merge_timestep_h_shard(0, 1, p, add_h=1, blur=0)):
                with pytest.raises(smk.SmkError, match=r"time step 0 \(the source\) has a valid halo of 2 voxels, the stencil reaches 2 .*>= 3 is needed"):
                    call()
    finally:
        C.close()
    # the nelts rules: a field and G at least; H besides; a u16 voxel holds three channels
    for rg, ne, add_h, why in (("u8", 1, 0, r"nelts 1: with add_h 0 a multi-field step is at least one field, G \(nelts >= 2\)"),
                               ("u8", 2, 1, r"nelts 2: with add_h 1 a multi-field step is at least one field, G and H \(nelts >= 3\)"),
                               ("u16", 2, 1, "add_h on a 16-bit ring of nelts 2: a u16 voxel holds three channels")):
        Fn = H.fields(rg, ne, dims, 0)
        C = gpu_renderer_factory()
        try:
            C.set_shard(0, nranks)
            C.set_option("halo", 3)
            C.set_timestep_cache(3)
            C.upload_volume(Fn, grad, fsize=fsz(dims), dmode="V1" if ne == 1 else "V1G")
            fp = [dev(np.ascontiguousarray(Fn[..., 0]))]
            for call in (lambda: C.step_extremes_h_device(0, p, add_h=add_h), lambda: C.merge_timestep_h_shard(0, 1, p, add_h=add_h),
                         lambda: C.block_extremes_h_device([fp[0][0]], CODE[rg], whole, p, add_h=add_h),
                         lambda: C.upload_timestep_fields_h_block_device(1, [fp[0][0]], CODE[rg], whole, p, add_h=add_h)):
                with pytest.raises(smk.SmkError, match=why):
                    call()
            assert C.timesteps() == (0, [0])
        finally:
            C.close()
    # no slot: a ring of one step, the current one
    one = declared(gpu_renderer_factory, dims, ring, 4, "V2GH", cap=1)
    try:
        with pytest.raises(smk.SmkError, match=r"smk_upload_timestep_fields_h_block_device: time step 5: the cache holds one step, the current one \(0\)"):
            one.upload_timestep_fields_h_block_device(5, ptrs, 0, whole, p)
        assert one.timesteps() == (0, [0]) and not one.download_timestep(0)[0].any()
    finally:
        one.close()
    # a sharded context still refuses the one-call entries, now naming the two-call forms
    C = rank_context(gpu_renderer_factory, dims, data, grad, "V2GH", 0, nranks, 3, cap=3)
    try:
        with pytest.raises(smk.SmkError, match=r"a sharded context.*reaches 2 voxels beyond region \+ halo.*three extremes.*smk_step_extremes_h_device \+ "
                                                 r"smk_merge_timestep_h_shard.*smk_block_extremes_h_device \+ smk_upload_timestep_fields_h_block_device"):
            C.merge_timestep_h(0, 1)
        assert C.timesteps() == (0, [0])
    finally:
        C.close()
    del held
