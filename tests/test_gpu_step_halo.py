"""Halo refill (smk.h: smk_step_halo_layout, smk_step_halo_exports_device, smk_step_halo_entries_device,
smk_step_halo_exchange_local; sortlast.refill_halo_local).  The yardstick everywhere is a TWIN: sharded contexts with the same
options that UPLOADED the unsharded result's voxels; the unsharded entry runs on one context and is downloaded.  Everything is
bit-exact.  The cases are tests/_step_halo_ref.py's (qualified by tests/test_step_halo_cpu.py): volumes of 3000 voxels."""
import ctypes

import numpy as np
import pytest

import _step_block_ref as B
import _step_halo_ref as HR
import _step_merge_h_ref as H
import _step_shard_ref as S
import _tblend_ref as T
import _step_gpu as G
from _gpu_mem import dev_ptr as dev, enqueue_layers, fetch_layers, layer_buffer, layers_of, out_buffer
from _step_gpu import (MODE, UndisturbedHalos, close, declared, dmode, flags_of, fsz, pert_scene, probe_at, rank_context,
                       ranks_declared, ranks_of, reference_of_arrays, reference_of_source, run_cut, same_bits as same)

pytestmark = pytest.mark.gpu
CODE = H.CODE


# ---- contexts, producers and twins

def declared_ranks(factory, dims, cls, nranks, halo):
    ring, nelts, normals = HR.CLASSES[cls]
    rs = []
    try:
        for r in range(nranks):
            rs.append(declared(factory, dims, ring, nelts, "VGH" if nelts == 3 else "V4", r, nranks, halo, normals))
    except Exception:
        close(rs)
        raise
    return rs


PRODUCERS = ("derive", "merge", "merge_h", "block_derive", "block_merge", "block_merge_h")
_RECIPE = {}


def recipe(factory, smk, prod, cls, dims):
    """(data mode, unsharded result data, its normals or None, make(nranks, halo, cap, opts) -> (ranks whose step 1 is the
    producer's, what must stay alive)).  The block forms take ghost cells of exactly the reach + 1"""
    from simian_spacemonkey_amd import sortlast
    key = (prod, cls, dims)
    if key in _RECIPE:
        return _RECIPE[key]
    ring, nelts, normals = HR.CLASSES[cls]
    if prod == "derive":
        data, grad, wdata, wgrad = reference_of_source(factory, "derive", ring, dims, compat=1, blur=1)[:4]
        dm = "VGH"

        def make(nranks, halo, cap=4, opts=()):
            rs = ranks_of(factory, dims, data, grad, "VGH", nranks, halo, cap, opts)
            return rs, sortlast.stencil_timestep_local(rs, "derive", 0, 1, compat=1, blur=1)
    elif prod == "merge":
        data, grad, wdata, wgrad = reference_of_source(factory, "merge", ring, dims, nf=nelts - 1, normals=normals)[:4]
        dm = MODE[nelts]

        def make(nranks, halo, cap=4, opts=()):
            rs = ranks_of(factory, dims, data, grad, dm, nranks, halo, cap, opts)
            return rs, sortlast.stencil_timestep_local(rs, "merge", 0, 1)
    elif prod == "merge_h":
        nf = nelts - 2
        data, grad = H.source_step(H.fields(ring, nf, dims, 0), 1)
        grad = grad if normals else None
        dm = H.MODE[(nf, 1)]
        U = rank_context(factory, dims, data, grad, dm)
        try:
            U.merge_timestep_h(0, 1, 1, 1, 1)
            wdata, wgrad = U.download_timestep(1)
        finally:
            U.close()

        def make(nranks, halo, cap=4, opts=()):
            rs = ranks_of(factory, dims, data, grad, dm, nranks, halo, cap, opts)
            return rs, sortlast.stencil_timestep_local(rs, "merge_h", 0, 1, compat=1, blur=1, add_h=1)
    elif prod in ("block_derive", "block_merge"):
        kind = prod[6:]
        nf = 2 if kind == "derive" else nelts - 1
        blur = 1 if kind == "derive" else 0
        arr, wdata, wgrad = reference_of_arrays(factory, kind, ring, dims, ring, nf, 1, blur, normals)[:3]
        dm = dmode(kind, nelts)

        def make(nranks, halo, cap=4, opts=()):
            cuts = [B.Cut(kind, dims, r, nranks, halo - B.WIDER, ring, "c") for r in range(nranks)]
            assert all(c.option_halo == halo for c in cuts)
            rs = ranks_declared(factory, dims, ring, nelts, dm, cuts, normals, cap, opts)
            try:
                return rs, run_cut(smk, rs, cuts, kind, ring, ring, arr, 1, 1, blur)
            except Exception:
                close(rs)
                raise
    else:
        nf = nelts - 2
        F = H.fields(ring, nf, dims, 0)
        arr = [np.ascontiguousarray(F[..., e]) for e in range(nf)]
        dm = H.MODE[(nf, 1)]
        held = [dev(a) for a in arr]
        U = declared(factory, dims, ring, nelts, dm, normals=normals)
        try:
            U.upload_timestep_fields_h_device(1, [h[0] for h in held], CODE[ring], dims, 1, 1, 1)
            wdata, wgrad = U.download_timestep(1)
        finally:
            U.close()
        del held

        def make(nranks, halo, cap=4, opts=()):
            cuts = [B.Cut("derive", dims, r, nranks, halo - B.WIDER, ring, "c", reach=2) for r in range(nranks)]
            rs = ranks_declared(factory, dims, ring, nelts, dm, cuts, normals, cap, opts)
            try:
                return rs, run_cut(smk, rs, cuts, "merge_h", ring, ring, arr, 1, 1, 1, add_h=1)
            except Exception:
                close(rs)
                raise
    wgrad = wgrad if normals else None
    _RECIPE[key] = (dm, wdata, wgrad, make)
    return _RECIPE[key]


def stored_cells(dims, r, nranks, halo, ring):
    """every probe cell of S_r, the box rank r stores cut at the volume"""
    g0, g1, O, Dd, pad = S.stored_box(dims, r, nranks, halo, ring)
    return S.cells_of(*S.uploaded_valid(dims, O, Dd))


def probes(rs, dims, halo, ring, step):
    return [R.probe_step(stored_cells(dims, r, len(rs), halo, ring), step) for r, R in enumerate(rs)]


_TWIN = {}


def twin_probes(factory, key, dims, wdata, wgrad, dm, nranks, halo, ring):
    """probe(every cell of S_r) of every rank of the twin, made once and shared"""
    k = (key, dims, nranks, halo)
    if k not in _TWIN:
        tw = ranks_of(factory, dims, wdata, wgrad, dm, nranks, halo)
        try:
            assert all(R.timestep_halo(0) == halo for R in tw)
            _TWIN[k] = probes(tw, dims, halo, ring, 0)
        finally:
            close(tw)
        assert all(p[2].all() for p in _TWIN[k]), "an uploaded step answers every cell of its stored box"
    return _TWIN[k]


def check_whole(rs, want, dims, halo, ring, step, what=""):
    for r, (R, (wraw, wnrm, _)) in enumerate(zip(rs, want)):
        raw, nrm, ok = R.probe_step(stored_cells(dims, r, len(rs), halo, ring), step)
        assert ok.all(), "%s rank %d: %d of %d cells of the stored box answered" % (what, r, ok.sum(), len(ok))
        same(raw, wraw, "%s rank %d: voxels of the stored box" % (what, r))
        same(nrm, wnrm, "%s rank %d: normals of the stored box" % (what, r))
        assert R.timestep_halo(step) == halo


def push(rs, sc):
    from _scenes import push_scene
    for R in rs:
        push_scene(R, sc, upload=False)


# ---- 1. the layout

@pytest.mark.parametrize("case", range(len(HR.CASES)), ids=HR.CASE_IDS)
def test_the_layout_is_the_models(gpu_renderer_factory, case):
    dims, nranks, halo = HR.CASES[case]
    for cls in HR.CLASSES:
        rs = declared_ranks(gpu_renderer_factory, dims, cls, nranks, halo)
        try:
            for r, R in enumerate(rs):
                got = R.step_halo_layout(nranks)
                assert got == HR.layout(dims, nranks, halo, cls, r), (cls, r, got, HR.layout(dims, nranks, halo, cls, r))
        finally:
            close(rs)


# ---- 2. refill after each producer

REFILLS = [("derive", "u8", 0), ("derive", "u16", 2), ("derive", "f32x3", 3),
           ("merge", "u8", 3), ("merge", "f32x4n", 1), ("merge", "f32x4", 4), ("merge", "u16", 5),
           ("merge_h", "u16", 6), ("merge_h", "f32x3", 0), ("merge_h", "f32x4n", 2),
           ("block_derive", "u8", 4), ("block_derive", "f32x3", 1),
           ("block_merge", "u16", 3), ("block_merge", "f32x4n", 0),
           ("block_merge_h", "u8", 2), ("block_merge_h", "f32x4", 3)]


@pytest.mark.parametrize("prod, cls, case", REFILLS, ids=["%s-%s-%s" % (p, c, HR.CASE_IDS[i]) for p, c, i in REFILLS])
def test_refill_after_each_producer(gpu_renderer_factory, smk, prod, cls, case):
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = HR.CASES[case]
    ring = HR.CLASSES[cls][0]
    dm, wdata, wgrad, make = recipe(gpu_renderer_factory, smk, prod, cls, dims)
    want = twin_probes(gpu_renderer_factory, (prod, cls), dims, wdata, wgrad, dm, nranks, halo, ring)
    rs, keep = make(nranks, halo)
    try:
        before = probes(rs, dims, halo, ring, 1)
        assert all(R.timestep_halo(1) < halo for R in rs)
        cut = [S.cut_anywhere(dims, *S.stored_box(dims, r, nranks, halo, ring)[2:4]) for r in range(nranks)]
        assert [not ok.all() for _, _, ok in before] == cut, "the witness: before the refill a rim cell is not answered"
        ids = [R.timesteps() for R in rs]
        sortlast.refill_halo_local(rs, 1)
        check_whole(rs, want, dims, halo, ring, 1, "%s %s" % (prod, cls))
        assert [R.timesteps() for R in rs] == ids, "the step keeps its id and its place in the ring"
        del keep
    finally:
        close(rs)


# ---- 3. the two-call form through explicit buffers

def all_to_all_v(rs, step, stream=None):
    """exports on every rank, the segments moved by device copies at the layout's offsets, entries on every rank"""
    import torch
    n = len(rs)
    lay = [R.step_halo_layout(n) for R in rs]
    exp = [out_buffer(max(l[2], 16), np.uint8, 0x5a) for l in lay]
    ent = [out_buffer(max(l[3], 16), np.uint8, 0xa5) for l in lay]
    for R, e in zip(rs, exp):
        R.step_halo_exports_device(e.data_ptr(), step, stream)
    torch.cuda.synchronize()                                # the exports ran on the contexts' streams; torch's copies do not wait for them
    for r in range(n):
        so = HR.offsets(lay[r][0])
        for j in range(n):
            ro = HR.offsets(lay[j][1])
            nb = lay[r][0][j]
            assert nb == lay[j][1][r]
            ent[j][ro[r]:ro[r] + nb].copy_(exp[r][so[j]:so[j] + nb])
    torch.cuda.synchronize()                                # ... and the contexts' streams do not wait for torch's copies
    for R, e in zip(rs, ent):
        R.step_halo_entries_device(e.data_ptr(), step, stream)
    torch.cuda.synchronize()                                # the entries are stored before the caller looks
    return exp, ent


@pytest.mark.parametrize("prod, cls, case", [("derive", "u8", 3), ("merge", "f32x4n", 2), ("merge_h", "u16", 0)])
def test_the_two_call_form_stores_the_local_forms_bits(gpu_renderer_factory, smk, prod, cls, case):
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = HR.CASES[case]
    ring = HR.CLASSES[cls][0]
    dm, wdata, wgrad, make = recipe(gpu_renderer_factory, smk, prod, cls, dims)
    want = twin_probes(gpu_renderer_factory, (prod, cls), dims, wdata, wgrad, dm, nranks, halo, ring)
    sc = pert_scene(np.ascontiguousarray(wdata[..., :3]), wgrad)
    opts = (("kernel", 1),)
    out = []
    for form in ("local", "buffers"):
        rs, keep = make(nranks, halo, opts=opts)
        try:
            if form == "local":
                sortlast.refill_halo_local(rs, 1)
            else:
                all_to_all_v(rs, 1)
            check_whole(rs, want, dims, halo, ring, 1, form)
            push(rs, sc)
            for R in rs:
                R.select_timestep(1)
            out.append(layers_of(rs, sc))
            del keep
        finally:
            close(rs)
    assert max(l[..., 3].max() for l in out[0]) > 0.01
    assert np.array_equal(out[0], out[1])


# ---- 4. brick summaries

def test_the_brick_summaries_are_made_again(gpu_renderer_factory):
    """Fields that stay above 100: under a table opaque for values near 0 alone, only the rim's zeros flag a brick.  The
    refill takes them away: the flags are the twin's, and differ from those before"""
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = (22, 13, 11), 4, 4
    rng = np.random.default_rng(11)
    data = rng.integers(100, 256, dims[::-1] + (3,)).astype(np.uint8)
    grad = rng.integers(0, 256, dims[::-1] + (3,)).astype(np.uint8)
    U = rank_context(gpu_renderer_factory, dims, data, grad, "V2G")
    try:
        U.merge_timestep(0, 1)
        wdata, wgrad = U.download_timestep(1)
    finally:
        U.close()
    assert wdata[..., 0].min() >= 100
    sc = T.scene(wdata, wgrad)
    table = np.zeros((256, 256, 4), np.uint8)
    table[:, :8] = 255                                      # ([sg][sv]: opaque where the first channel is below 8, whatever the second)
    opts = (("kernel", 1),)
    tw = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, "V2G", nranks, halo, opts=opts)
    try:
        want = [flags_of(R, sc, 0, [table])[0] for R in tw]
    finally:
        close(tw)
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "V2G", nranks, halo, opts=opts)
    try:
        keep = sortlast.stencil_timestep_local(rs, "merge", 0, 1)
        before = [flags_of(R, sc, 1, [table])[0] for R in rs]
        sortlast.refill_halo_local(rs, 1)
        after = [flags_of(R, sc, 1, [table])[0] for R in rs]
        del keep
    finally:
        close(rs)
    for r in range(nranks):
        assert np.array_equal(after[r], want[r]), "rank %d: %d bricks differ from the twin's" % (r, (after[r] != want[r]).sum())
        assert not np.array_equal(before[r], after[r]), "rank %d: the rim's zeros flagged no brick" % r
    assert not any(w.any() for w in want) and all(b.any() for b in before)


# ---- 5. the pinned refusal turned round

def shadow_layers(rs, sc):
    from simian_spacemonkey_amd.binding import shadow_exchange_local
    shadow_exchange_local(rs)
    return layers_of(rs, sc)


@pytest.mark.parametrize("nranks", [2, 8])
def test_the_refused_frames_render_after_the_refill(gpu_renderer_factory, smk, nranks):
    """the scene of test_gpu_step_shard.py::test_a_frame_compares_its_need_with_the_shown_steps_valid_halo: 21 x 13 x 11, halo 3,
    derived to valid halo 1.  The perturbed frame (and on two ranks the frame with shadows) is refused before the refill and is
    the twin's, layer by layer, after it"""
    from simian_spacemonkey_amd import sortlast
    dims, halo = (21, 13, 11), 3
    data, grad, wdata, wgrad, _, _ = reference_of_source(gpu_renderer_factory, "derive", "u8", dims)
    sc = pert_scene(wdata, wgrad)
    assert G.pert_need(dims, sc.pert_w)[0] == 2
    opts = (("kernel", 1),)
    shadows = nranks == 2

    def both(rs):
        push(rs, sc)
        out = [layers_of(rs, sc)]
        if shadows:
            for R in rs:
                R.set_shadow(1, 64, 0.75)
                R.set_perturb(None, None, None)
            need = [R.shadow_margin()[1] for R in rs]
            assert 1 < min(need) and max(need) <= halo, need
            out.append(shadow_layers(rs, sc))
        return out
    tw = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, "VGH", nranks, halo, opts=opts)
    try:
        want = both(tw)
    finally:
        close(tw)
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "VGH", nranks, halo, opts=opts)
    try:
        push(rs, sc)
        keep = sortlast.stencil_timestep_local(rs, "derive", 0, 1)
        for R in rs:
            R.select_timestep(1)
            assert R.timestep_halo() == 1
            with pytest.raises(smk.SmkError, match=r"perturbation needs halo >= 2 voxels .*time step 1 has a valid halo of 1, of option halo 3"):
                R.render()
        if shadows:
            for R in rs:
                R.set_shadow(1, 64, 0.75)
                R.set_perturb(None, None, None)
            with pytest.raises(smk.SmkError, match=r"shadows on a shard need halo >= \d+ voxels \(time step 1 has a valid halo of 1, of option halo 3"):
                sortlast.render_shadow_frame_local(rs)
        sortlast.refill_halo_local(rs, 1)
        assert all(R.timestep_halo() == halo for R in rs)
        got = both(rs)
        del keep
    finally:
        close(rs)
    for g, w, what in zip(got, want, ("perturbed", "shadows")):
        assert max(l[..., 3].max() for l in w) > 0.01, what
        for r in range(nranks):
            assert np.array_equal(g[r], w[r]), "%s, rank %d: max diff %g" % (what, r, np.abs(g[r] - w[r]).max())


# ---- 6. a second stencil on the refilled step

@pytest.mark.parametrize("ring", ["u8", "f32"])
def test_a_second_stencil_on_the_refilled_step(gpu_renderer_factory, smk, ring):
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = (22, 13, 11), 4, 4
    data, grad = S.source("derive", ring, dims)
    cells = S.cells_of((0, 0, 0), dims)
    U = rank_context(gpu_renderer_factory, dims, data, grad, "VGH")
    try:
        U.derive_timestep(0, 1, 1, 1)
        U.derive_timestep(1, 2, 1, 0)
        want = U.probe_step(cells, 2)
    finally:
        U.close()
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "VGH", nranks, halo)
    try:
        keep = [sortlast.stencil_timestep_local(rs, "derive", 0, 1, compat=1, blur=1)]
        with pytest.raises(smk.SmkError, match=r"time step 1 \(the source\) has a valid halo of 2 voxels, the stencil reaches 2"):
            sortlast.stencil_timestep_local(rs, "derive", 1, 2, compat=1, blur=0)
        sortlast.refill_halo_local(rs, 1)
        keep.append(sortlast.stencil_timestep_local(rs, "derive", 1, 2, compat=1, blur=0))
        for r, R in enumerate(rs):
            g0, g1, O, Dd, pad = S.stored_box(dims, r, nranks, halo, ring)
            assert [R.timestep_halo(t) for t in (0, 1, 2)] == [halo, halo, halo - 2]
            lo, hi = S.valid_box(dims, O, Dd, 2)            # (shrunk once, from the whole stored box: the refill undid the first)
            cs = S.cells_of(*S.uploaded_valid(dims, O, Dd))
            raw, nrm, ok = R.probe_step(cs, 2)
            inside = np.all((cs >= np.array(lo)) & (cs + 1 < np.array(hi)), -1)
            assert np.array_equal(ok, inside) and (S.straddles(cs, g0, g1) & inside).any()
            wraw, wnrm = probe_at(want, dims, cs[inside])
            same(raw[inside], wraw, "rank %d: the chain's voxels" % r)
            same(nrm[inside], wnrm, "rank %d: the chain's normals" % r)
        del keep
    finally:
        close(rs)


# ---- 7. ordering

def test_refill_and_frames_on_one_stream_without_a_host_wait(gpu_renderer_factory, smk):
    """producer, refill and frame enqueued on a caller's stream; then the CURRENT step refilled between two frames; then an
    upload into the slot on another stream right behind an export"""
    import torch
    from simian_spacemonkey_amd import sortlast
    from simian_spacemonkey_amd.binding import STEP_CURRENT
    dims, nranks, halo, ring = (21, 13, 11), 2, 3, "u8"
    data, grad, wdata, wgrad, _, _ = reference_of_source(gpu_renderer_factory, "derive", ring, dims)
    data2, grad2 = S.source("derive", ring, dims, seed=1)
    plain, pert = T.scene(wdata, wgrad), pert_scene(wdata, wgrad)
    opts = (("kernel", 1),)
    tw = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, "VGH", nranks, halo, opts=opts)
    try:
        push(tw, plain)
        want_plain = layers_of(tw, plain)
        push(tw, pert)
        want_pert = layers_of(tw, pert)
    finally:
        close(tw)
    assert not np.array_equal(want_plain, want_pert)
    side, other = torch.cuda.Stream(), torch.cuda.Stream()
    st, ot = ctypes.c_void_p(side.cuda_stream), ctypes.c_void_p(other.cuda_stream)
    # (a) one stream, no host wait between the write pass, the refill and the frames
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "VGH", nranks, halo, opts=opts)
    try:
        push(rs, pert)
        layers = layer_buffer(rs, pert)
        keep = sortlast.stencil_timestep_local(rs, "derive", 0, 1, stream=st)
        for R in rs:
            R.select_timestep(1)
        sortlast.refill_halo_local(rs, 1, stream=st)
        enqueue_layers(rs, layers, st)
        got = fetch_layers(layers, pert)
        assert np.array_equal(got, want_pert)
        # (c) an export, and right behind it an upload into the slot on another stream: the export holds the old step's voxels
        lay = rs[0].step_halo_layout(nranks)
        calm = out_buffer(lay[2], np.uint8)
        busy = out_buffer(lay[2], np.uint8)
        pd, k0 = dev(data2)
        pg, k1 = dev(grad2)
        rs[0].step_halo_exports_device(calm.data_ptr(), 1)
        torch.cuda.synchronize()                            # the calm export has ended before the busy one and the upload start
        rs[0].step_halo_exports_device(busy.data_ptr(), 1, st)
        rs[0].upload_timestep_device(1, pd, dims, 3, CODE[ring], pg, fsize=fsz(dims), dmode="VGH", stream=ot)
        torch.cuda.synchronize()                            # both streams: read-back
        assert calm.any() and torch.equal(calm, busy)
        g0, g1 = S.stored_box(dims, 0, nranks, halo, ring)[:2]
        same(rs[0].download_timestep(1)[0], data2[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]], "the upload behind the export")
        del keep, k0, k1
    finally:
        close(rs)
    # (b) the CURRENT step refilled between two frames
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "VGH", nranks, halo, opts=opts)
    try:
        push(rs, plain)
        l1, l2 = layer_buffer(rs, plain), layer_buffer(rs, pert)
        keep = sortlast.stencil_timestep_local(rs, "derive", 0, 1, stream=st)
        for R in rs:
            R.select_timestep(1)
        enqueue_layers(rs, l1, st)
        sortlast.refill_halo_local(rs, STEP_CURRENT, stream=st)
        push(rs, pert)
        enqueue_layers(rs, l2, st)
        first, second = fetch_layers(l1, plain), fetch_layers(l2, pert)
        assert all(R.timesteps() == (1, [0, 1]) and R.timestep_halo() == halo for R in rs)
        del keep
    finally:
        close(rs)
    assert np.array_equal(first, want_plain), "a frame that needs one halo voxel, before the refill"
    assert np.array_equal(second, want_pert)


# ---- 8. idempotence, the unsharded no-op, refusals

@pytest.mark.parametrize("cls", ["u8", "f32x4n"])
def test_idempotent_on_an_uploaded_step(gpu_renderer_factory, cls):
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = HR.CASES[3]
    ring, nelts, normals = HR.CLASSES[cls]
    data, grad = S.source("merge", ring, dims, nf=nelts - 1)
    sc = pert_scene(np.ascontiguousarray(data[..., :3]), grad)
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, MODE[nelts], nranks, halo, opts=(("kernel", 1),))
    try:
        push(rs, sc)
        p0 = probes(rs, dims, halo, ring, 0)
        f0 = layers_of(rs, sc)
        sortlast.refill_halo_local(rs, 0)
        check_whole(rs, p0, dims, halo, ring, 0, "after one refill")
        f1 = layers_of(rs, sc)
        all_to_all_v(rs, 0)
        check_whole(rs, p0, dims, halo, ring, 0, "after the two-call form")
        f2 = layers_of(rs, sc)
    finally:
        close(rs)
    assert max(l[..., 3].max() for l in f0) > 0.01
    assert np.array_equal(f0, f1) and np.array_equal(f0, f2)


def test_an_unsharded_context_has_nothing_to_refill(gpu_renderer_factory):
    from simian_spacemonkey_amd import sortlast
    dims = (21, 13, 11)
    data, grad = S.source("derive", "u8", dims)
    sc = T.scene(data, grad)
    U = rank_context(gpu_renderer_factory, dims, data, grad, "VGH")
    try:
        push([U], sc)
        f0, d0 = U.render(), U.download_timestep(0)
        assert U.step_halo_layout(1) == ([0], [0], 0, 0)
        U.step_halo_exports_device(None, 0)
        U.step_halo_entries_device(None, 0)
        sortlast.refill_halo_local([U], 0)
        assert U.timestep_halo(0) == 1 and U.timesteps() == (0, [0])
        f1, d1 = U.render(), U.download_timestep(0)
    finally:
        U.close()
    assert np.array_equal(f0, f1)
    same(d1[0], d0[0], "data")
    same(d1[1], d0[1], "normals")


def test_refusals_change_nothing(gpu_renderer_factory, smk):
    import torch
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo = (21, 13, 11), 2, 3
    data, grad = S.source("derive", "u8", dims)
    sc = T.scene(data, grad)
    buf = out_buffer(1 << 16, np.uint8, 0x5a)
    p = buf.data_ptr()
    E = smk.SmkError
    C = gpu_renderer_factory()
    try:
        C.set_shard(0, 2)
        for call, who in ((lambda: C.step_halo_layout(2), "smk_step_halo_layout"), (lambda: C.step_halo_exports_device(p, 0), "smk_step_halo_exports_device"),
                          (lambda: C.step_halo_entries_device(p, 0), "smk_step_halo_entries_device")):
            with pytest.raises(E, match=who + ": no volume"):
                call()
    finally:
        C.close()
    opts = (("kernel", 1),)
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "VGH", nranks, halo, opts=opts)
    odd = []
    try:
        push(rs, sc)
        keep = sortlast.stencil_timestep_local(rs, "derive", 0, 1)
        f32 = data.astype(np.float32)
        for dd, gg, dg, h, dm in (((22, 13, 11), None, None, halo, "VGH"), (dims, f32, grad, halo, "VGH"), (dims, data[..., :2], grad, halo, "V1G"),
                                  (dims, data, None, halo, "VGH"), (dims, data, grad, halo + 1, "VGH")):
            if gg is None and dd != dims:
                gg, dg = S.source("derive", "u8", dd)
            R = gpu_renderer_factory()
            odd.append(R)
            R.set_shard(1, nranks)
            R.set_option("halo", h)
            R.set_timestep_cache(4)
            R.upload_volume(np.ascontiguousarray(gg), dg, fsize=fsz(dd), dmode=dm)
            R.upload_timestep(1, np.ascontiguousarray(gg), dg, fsize=fsz(dd), dmode=dm)
        with UndisturbedHalos(rs[0], downloads=False), UndisturbedHalos(rs[1], downloads=False):
            before = probes(rs, dims, halo, "u8", 1)
            for call, why in (
                    (lambda: rs[0].step_halo_exports_device(p, 99), "smk_step_halo_exports_device: time step 99 is not cached"),
                    (lambda: rs[0].step_halo_entries_device(p, 99), "smk_step_halo_entries_device: time step 99 is not cached"),
                    (lambda: sortlast.refill_halo_local(rs, 99), "smk_step_halo_exchange_local: time step 99 is not cached"),
                    (lambda: rs[0].step_halo_exports_device(None, 1), "smk_step_halo_exports_device: d_exports is NULL and"),
                    (lambda: rs[0].step_halo_entries_device(None, 1), "smk_step_halo_entries_device: d_entries is NULL and"),
                    (lambda: rs[0].step_halo_exports_device(p + 8, 1), "d_exports is not aligned to 16 bytes"),
                    (lambda: rs[0].step_halo_entries_device(p + 8, 1), "d_entries is not aligned to 16 bytes"),
                    (lambda: sortlast.refill_halo_local(rs[:1], 1), "context 0 is not shard 0 of 1"),
                    (lambda: sortlast.refill_halo_local(rs[::-1], 1), "context 0 is not shard 0 of 2"),
                    (lambda: sortlast.refill_halo_local([rs[0], odd[0]], 1), "rank 1 differs from rank 0 in dims: 22x13x11, not 21x13x11"),
                    (lambda: sortlast.refill_halo_local([rs[0], odd[1]], 1), "rank 1 differs from rank 0 in dtype: 1, not 0"),
                    (lambda: sortlast.refill_halo_local([rs[0], odd[2]], 1), "rank 1 differs from rank 0 in nelts: 2, not 3"),
                    (lambda: sortlast.refill_halo_local([rs[0], odd[3]], 1), "rank 1 differs from rank 0 in normals: absent, not present"),
                    (lambda: sortlast.refill_halo_local([rs[0], odd[4]], 1), "rank 1 differs from rank 0 in halo: 4, not 3")):
                with pytest.raises(E, match=why):
                    call()
            torch.cuda.synchronize()                        # the contexts' streams: read-back
            assert (buf.cpu().numpy() == 0x5a).all(), "a refused export writes no byte"
            after = probes(rs, dims, halo, "u8", 1)
            for (r0, n0, k0), (r1, n1, k1) in zip(before, after):
                assert np.array_equal(k0, k1) and not k0.all()
                same(r1, r0, "voxels after the refusals")
                same(n1, n0, "normals after the refusals")
            assert all(R.timestep_halo(1) == 1 for R in rs)
        del keep
    finally:
        close(rs + odd)
