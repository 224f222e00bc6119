"""The stencil producers on sharded contexts (smk.h: smk_step_extremes_device, smk_derive_timestep_shard,
smk_merge_timestep_shard, smk_get_timestep_halo).  Expected values come from the EXISTING one-call entries, smk_derive_timestep
and smk_merge_timestep, run in the same test on an unsharded context that holds the same step: the ranks' words, regions,
halo voxels and frames must be that context's, bit for bit.  The cases are tests/_step_shard_ref.py's (qualified by
tests/test_step_shard_cpu.py): volumes of a few ten thousand voxels."""
import ctypes

import numpy as np
import pytest

import _step_shard_ref as S
import _tblend_ref as T
from _gpu_mem import dev_ptr as dev, merged, words_buf
from _step_gpu import (RAN, SORT_LAST_TOL, UndisturbedHalos as Undisturbed, close, dmode, export, fsz, one_call, params, pert_need, pert_scene,
                       probe_at, rank_context, ranks_of, reference_of_source as reference, same_bits as same, write_shard)

pytestmark = pytest.mark.gpu
CASES = [pytest.param(i, ring, id="%s-%s" % (S.CASE_IDS[i], ring)) for i in range(len(S.CASES)) for ring in S.RINGS]


# ---- 1. the words

@pytest.mark.parametrize("case, ring", CASES)
def test_the_ranks_words_combine_to_the_unsharded_words(gpu_renderer_factory, case, ring):
    kind, dims, nranks, halo = S.CASES[case]
    compat, _ = params(kind, case)
    data, grad, _, _, want, _ = reference(gpu_renderer_factory, kind, ring, dims, compat=compat, blur=params(kind, case)[1])
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), nranks, halo)
    try:
        words = [export(R, kind, 0, compat) for R in rs]
    finally:
        close(rs)
    assert np.array_equal(S.combine(words), want), (words, want)
    assert (want[6 if kind == "derive" else 1:] == S.INT_MIN).all() and not np.array_equal(want, S.SEEDS[kind])
    for r, w in enumerate(words):
        g0, g1, _, _, _ = S.stored_box(dims, r, nranks, halo, ring)
        if not S.has_interior(dims, g0, g1):
            assert np.array_equal(w, S.SEEDS[kind]), "rank %d has no interior voxel: %s" % (r, w)
        else:
            assert not np.array_equal(w, S.SEEDS[kind])


# ---- 2. the two-call form on an unsharded context

TWO_CALL = [(kind, ring, nf, kernel) for kind, ring, nf in (("derive", "u8", 2), ("derive", "u16", 2), ("derive", "f32", 2), ("merge", "u8", 3),
                                                             ("merge", "u16", 2), ("merge", "f32", 2)) for kernel in (1, 2)]
TWO_CALL.append(("merge", "f32", 3, 1))                     # (four-channel f32 voxels: the gather kernel alone renders them)


@pytest.mark.parametrize("kind, ring, nf, kernel", TWO_CALL)
def test_export_and_write_on_an_unsharded_context_is_the_one_call_entry(gpu_renderer_factory, kind, ring, nf, kernel):
    from _scenes import push_scene
    dims = (37, 13, 11)                                     # (odd x and y: a pad column and row of 8-byte voxels)
    data, grad = S.source(kind, ring, dims, nf)
    sc = T.scene(np.ascontiguousarray(data[..., :3]), grad)
    R = rank_context(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), opts=(("kernel", kernel),))
    try:
        push_scene(R, sc, upload=False)
        one_call(R, kind, 0, 1, 1, 1)
        w = words_buf()
        R.step_extremes_device(0 if kind == "derive" else 1, 0, w.data_ptr())
        write_shard(R, kind, 0, 2, w.data_ptr(), 1, 1)
        assert R.timestep_halo(1) == R.timestep_halo(2) == R.timestep_halo(0) == 1
        a, b = R.download_timestep(1), R.download_timestep(2)
        same(b[0], a[0], "data")
        same(b[1], a[1], "normals")
        assert not np.array_equal(a[0], R.download_timestep(0)[0])
        frames = []
        for t in (1, 2):
            R.select_timestep(t)
            frames.append(R.render())
            assert R.last_frame_info()[0] == RAN[kernel]
        assert R.stat("slab_failures") == 0
    finally:
        R.close()
    assert frames[0][..., 3].max() > 0.05
    assert np.array_equal(frames[0], frames[1]), np.abs(frames[0] - frames[1]).max()


# ---- 3. the regions, 4. the halo and the rim, and the valid halo of the result

def check_ranks(factory, kind, ring, dims, nranks, halo, nf=2, compat=1, blur=0, normals=True):
    from simian_spacemonkey_amd import sortlast
    data, grad, wdata, wgrad, wwords, wprobe = reference(factory, kind, ring, dims, nf, compat, blur, normals)
    reach = S.REACH[kind]
    rs = ranks_of(factory, dims, data, grad, dmode(kind, data.shape[-1]), nranks, halo)
    try:
        words = sortlast.stencil_timestep_local(rs, kind, 0, 1, compat=compat, blur=blur)
        assert np.array_equal(words.cpu().numpy()[nranks], wwords)
        parts, gparts = [], []
        for r, R in enumerate(rs):
            g0, g1, O, Dd, pad = S.stored_box(dims, r, nranks, halo, ring)
            origin, size, ne, dt, hn = R.timestep_box()
            assert origin == g0 and size == tuple(b - a for a, b in zip(g0, g1)) and hn == normals
            got = R.download_timestep(1)
            parts.append((origin, got[0]))
            gparts.append((origin, got[1]))
            assert R.timestep_halo(0) == halo and R.timestep_halo(1) == halo - reach
            assert R.timesteps() == (0, [0, 1])
            # every cell of the stored box that lies in the volume: answered inside the valid box, and only there
            lo, hi = S.valid_box(dims, O, Dd, reach)
            slo, shi = S.uploaded_valid(dims, O, Dd)
            cells = S.cells_of(slo, shi)
            raw, nrm, ok = R.probe_step(cells, 1)
            inside = np.all((cells >= np.array(lo)) & (cells + 1 < np.array(hi)), -1)
            assert np.array_equal(ok, inside), "rank %d: %d cells answered, %d lie in the valid box" % (r, ok.sum(), inside.sum())
            assert R.probe_step(cells, 0)[2].all(), "the uploaded source answers every cell of the stored box"
            st = S.straddles(cells, g0, g1) & inside
            assert st.any() or nranks == 1
            wraw, wnrm = probe_at(wprobe, dims, cells[inside])
            same(raw[inside], wraw, "rank %d: the valid box's voxels" % r)
            same(nrm[inside], wnrm, "rank %d: the valid box's normals" % r)
            assert not raw[~inside].any() and not nrm[~inside].any()
    finally:
        close(rs)
    same(S.place(dims, wdata.shape[-1], wdata.dtype, parts), wdata, "data")
    same(S.place(dims, 3, np.uint8, gparts), wgrad, "normals")
    if not normals:
        assert (wgrad == 128).all()


@pytest.mark.parametrize("case, ring", CASES)
def test_the_ranks_regions_and_halos_are_the_unsharded_step(gpu_renderer_factory, case, ring):
    kind, dims, nranks, halo = S.CASES[case]
    compat, blur = params(kind, case)
    check_ranks(gpu_renderer_factory, kind, ring, dims, nranks, halo, compat=compat, blur=blur)


@pytest.mark.parametrize("ring, nf", [("u8", 1), ("u8", 3), ("u16", 1), ("f32", 1), ("f32", 3)])
def test_merge_of_one_to_three_fields(gpu_renderer_factory, ring, nf):
    """(two fields: every merge case above; f32 with three fields keeps its normals in the separate buffer)"""
    check_ranks(gpu_renderer_factory, "merge", ring, (74, 21, 19), 4, 3, nf=nf)


@pytest.mark.parametrize("kind, ring, nf", [("derive", "u8", 2), ("derive", "f32", 2), ("merge", "u16", 2), ("merge", "f32", 3)])
def test_a_context_without_normals(gpu_renderer_factory, kind, ring, nf):
    check_ranks(gpu_renderer_factory, kind, ring, (75, 21, 19), 2, 3, nf=nf, normals=False)


# ---- 5. frames

@pytest.mark.parametrize("bricks", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2], ids=["gather", "slice-ring"])
@pytest.mark.parametrize("kind, ring, halo", [("derive", "u8", 3), ("derive", "f32", 4), ("merge", "u16", 2)])
def test_frames_of_the_produced_step(gpu_renderer_factory, kind, ring, halo, kernel, bricks):
    from _scenes import push_scene
    from simian_spacemonkey_amd import sortlast
    dims, nranks = (75, 21, 19), 2
    data, grad, wdata, wgrad, _, _ = reference(gpu_renderer_factory, kind, ring, dims)
    opts = (("kernel", kernel), ("bricks", bricks), ("slab_split", 1))
    sc = T.scene(wdata, wgrad)

    def frames(rs):
        for R in rs:
            push_scene(R, sc, upload=False)
        lay, out = merged(rs, sc)
        assert all(R.last_frame_info()[0] == RAN[kernel] for R in rs) and all(R.stat("slab_failures") == 0 for R in rs)
        return lay, out
    up = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, dmode(kind, wdata.shape[-1]), nranks, halo, opts=opts)      # ... that UPLOADED the unsharded result
    try:
        want_layers, want = frames(up)
    finally:
        close(up)
    U = rank_context(gpu_renderer_factory, dims, wdata, wgrad, dmode(kind, wdata.shape[-1]), opts=opts)
    try:
        push_scene(U, sc, upload=False)
        whole = U.render()
    finally:
        U.close()
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), nranks, halo, opts=opts)
    try:
        frames(rs)                                          # (the source rendered first: flags and plans of another step exist)
        keep = sortlast.stencil_timestep_local(rs, kind, 0, 1)
        for R in rs:
            R.select_timestep(1)
        got_layers, got = frames(rs)
        del keep
    finally:
        close(rs)
    assert whole[..., 3].max() > 0.05 and all(l[..., 3].max() > 0.01 for l in want_layers)
    for r in range(nranks):
        assert np.array_equal(got_layers[r], want_layers[r]), "rank %d: max diff %g" % (r, np.abs(got_layers[r] - want_layers[r]).max())
    assert np.array_equal(got, want)                        # (tests/test_gpu_timesteps.py: merged shards against fresh shards, exactly)
    err = np.abs(got - whole).max()
    assert err <= SORT_LAST_TOL, "merged against the unsharded frame: max abs err %g" % err


# ---- 6. the valid halo

def test_the_valid_halo_follows_uploads_blends_and_stencils(gpu_renderer_factory, smk):
    dims, nranks, halo = (75, 21, 19), 2, 3
    data, grad = S.source("derive", "u8", dims)
    data2, grad2 = S.source("derive", "u8", dims, seed=1)
    R = rank_context(gpu_renderer_factory, dims, data, grad, "VGH", 1, nranks, halo, cap=6)
    try:
        R.upload_timestep(1, data2, grad2, fsize=fsz(dims), dmode="VGH")
        R.blend_timesteps(0, 1, 0.4, 2)
        assert [R.timestep_halo(t) for t in (0, 1, 2)] == [3, 3, 3] and R.timestep_halo() == 3
        w = words_buf()
        R.step_extremes_device(1, 2, w.data_ptr())          # (a lone rank: its own words are all it combines)
        R.merge_timestep_shard(2, 3, w.data_ptr())
        assert R.timestep_halo(3) == 2
        R.step_extremes_device(0, 2, w.data_ptr())
        R.derive_timestep_shard(2, 4, w.data_ptr())
        assert R.timestep_halo(4) == 1
        R.blend_timesteps(3, 4, 0.5, 5)
        assert R.timestep_halo(5) == 1, "a blend keeps the smaller of its sources' valid halos"
        before = R.timesteps()
        for call in (lambda: R.step_extremes_device(0, 4, w.data_ptr()), lambda: R.derive_timestep_shard(4, 0, w.data_ptr()),
                     lambda: R.derive_timestep_shard(3, 0, w.data_ptr())):
            with pytest.raises(smk.SmkError, match=r"valid halo of [12] voxels, the stencil reaches 2 .* valid halo >= 3 is needed"):
                call()
        with pytest.raises(smk.SmkError, match=r"smk_derive_timestep_shard: time step 4 \(the source\) has a valid halo of 1 voxels"):
            R.derive_timestep_shard(4, 0, w.data_ptr())
        R.merge_timestep_shard(3, 0, w.data_ptr())          # (valid halo 2 = reach + 1: allowed; the current step overwritten in place)
        assert R.timestep_halo(0) == 1 and R.timesteps()[0] == before[0]
        with pytest.raises(smk.SmkError, match="smk_get_timestep_halo: time step 77 is not cached"):
            R.timestep_halo(77)
    finally:
        R.close()


@pytest.mark.parametrize("halo, renders", [(3, False), (4, True)])
def test_a_frame_compares_its_need_with_the_shown_steps_valid_halo(gpu_renderer_factory, smk, halo, renders):
    from _scenes import push_scene
    from simian_spacemonkey_amd import sortlast
    dims, nranks = (21, 13, 11), 2
    data, grad, wdata, wgrad, _, _ = reference(gpu_renderer_factory, "derive", "u8", dims)
    sc = pert_scene(wdata, wgrad)
    need = pert_need(dims, sc.pert_w)
    assert need[0] == 2                                     # x is the split axis: halo 3 - reach 2 < 2 <= halo 4 - reach 2
    opts = (("kernel", 1),)
    rs = ranks_of(gpu_renderer_factory, dims, data, grad, "VGH", nranks, halo, opts=opts)
    try:
        for R in rs:
            push_scene(R, sc, upload=False)
        _, uploaded = merged(rs, sc)                        # the uploaded source has halo >= need: it renders
        keep = sortlast.stencil_timestep_local(rs, "derive", 0, 1)
        for R in rs:
            R.select_timestep(1)
            assert R.timestep_halo() == halo - 2
        if not renders:
            for R in rs:
                with pytest.raises(smk.SmkError, match=r"perturbation needs halo >= 2 voxels .*time step 1 has a valid halo of 1, of option halo 3"):
                    R.render()
                R.set_shadow(1, 64, 0.75)
                R.set_perturb(None, None, None)
            # the shadow margin against the same number (phase 1 of the light exchange).  The margin is at least one voxel
            # (smk_get_shadow_margin rounds up), so halo_needed >= 2 exceeds the derived step's valid halo of 1
            assert min(R.shadow_margin()[1] for R in rs) > 1
            with pytest.raises(smk.SmkError, match=r"shadows on a shard need halo >= \d+ voxels \(time step 1 has a valid halo of 1, of option halo 3"):
                sortlast.render_shadow_frame_local(rs)
            for R in rs:
                R.set_shadow(0)
                R.select_timestep(0)
                R.render()                                  # (the source is shown again: its halo is whole)
            return
        got_layers, got = merged(rs, sc)
        del keep
    finally:
        close(rs)
    up = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, "VGH", nranks, halo, opts=opts)
    try:
        for R in up:
            push_scene(R, sc, upload=False)
        want_layers, want = merged(up, sc)
    finally:
        close(up)
    assert want[..., 3].max() > 0.05 and not np.array_equal(want, uploaded)
    assert np.array_equal(got_layers, want_layers) and np.array_equal(got, want)


# ---- 7. refusals and the ring's rule

@pytest.mark.parametrize("kind", ["derive", "merge"])
def test_refusals_leave_the_ring_unchanged(gpu_renderer_factory, smk, kind):
    from _scenes import push_scene
    dims, nranks = (37, 13, 11), 2
    reach = S.REACH[kind]
    entry = "smk_%s_timestep_shard" % kind
    code = 0 if kind == "derive" else 1
    data, grad = S.source(kind, "u8", dims)
    data2, grad2 = S.source(kind, "u8", dims, seed=1)
    sc = T.scene(data, grad)
    w = words_buf()
    p = w.data_ptr()
    R = gpu_renderer_factory()
    try:
        with pytest.raises(smk.SmkError, match=entry + ": no volume"):
            write_shard(R, kind, 0, 1, p)
        with pytest.raises(smk.SmkError, match="smk_step_extremes_device: no volume"):
            R.step_extremes_device(code, 0, p)
    finally:
        R.close()
    # a ring of two slots, both held: the source and the current step leave no slot for the output
    R = rank_context(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), 0, nranks, reach + 1, cap=2, opts=(("kernel", 1),))
    try:
        push_scene(R, sc, upload=False)
        R.upload_timestep(1, data2, grad2, fsize=fsz(dims), dmode=dmode(kind, 3))
        with Undisturbed(R):
            for call, why in (
                    (lambda: write_shard(R, kind, 99, 5, p), entry + r": time step 99 \(the source\) is not cached"),
                    (lambda: write_shard(R, kind, -1, 5, p), "is not cached"),
                    (lambda: write_shard(R, kind, 0, -1, p), "ids are >= 0"),
                    (lambda: write_shard(R, kind, 1, 1, p), "in-place"),
                    (lambda: write_shard(R, kind, 1, 5, p), entry + r": the cache holds 2 steps.*here 3"),
                    (lambda: write_shard(R, kind, 1, 5, None), "d_words is NULL"),
                    (lambda: write_shard(R, kind, 1, 5, p + 2), "d_words is not aligned"),
                    (lambda: R.step_extremes_device(7, 0, p), "smk_step_extremes_device: kind 7 is neither"),
                    (lambda: R.step_extremes_device(code, 99, p), r"smk_step_extremes_device: time step 99 \(the source\) is not cached"),
                    (lambda: R.step_extremes_device(code, 0, None), "d_words is NULL")):
                with pytest.raises(smk.SmkError, match=why):
                    call()
        assert (w.cpu().numpy() == 0x5a5a5a5a).all(), "a refused export writes no word"
    finally:
        R.close()
    # the source's valid halo below reach + 1
    R = rank_context(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), 0, nranks, reach, cap=3, opts=(("kernel", 1),))
    try:
        push_scene(R, sc, upload=False)
        with Undisturbed(R):
            for call in (lambda: write_shard(R, kind, 0, 1, p), lambda: R.step_extremes_device(code, 0, p)):
                with pytest.raises(smk.SmkError, match=r"time step 0 \(the source\) has a valid halo of %d voxels, the stencil reaches %d .*>= %d is needed"
                                   % (reach, reach, reach + 1)):
                    call()
    finally:
        R.close()
    # the nelts rules
    ne = 2 if kind == "derive" else 1                       # (two channels are no VGH step; one channel is no field and G)
    R = gpu_renderer_factory()
    try:
        R.set_shard(0, nranks)
        R.set_option("halo", 3)
        R.set_timestep_cache(3)
        R.upload_volume(np.ascontiguousarray(data[..., :ne]), grad, fsize=fsz(dims), dmode="V1G" if ne == 2 else "V1")
        why = "nelts 2: V, G and H are three channels" if kind == "derive" else "nelts 1: a multi-field step is at least one field and G"
        for call in (lambda: write_shard(R, kind, 0, 1, p), lambda: R.step_extremes_device(code, 0, p)):
            with pytest.raises(smk.SmkError, match=why):
                call()
        assert R.timesteps() == (0, [0])
    finally:
        R.close()


# ---- 8. streams

@pytest.mark.parametrize("kind", ["derive", "merge"])
def test_on_a_stream_of_the_callers(gpu_renderer_factory, kind):
    """export, combine and write on a non-default stream, then an upload over the source on another stream and a frame: the
    upload waits for the producers' reads on the device, and the bits are those of the context's own stream"""
    import torch
    from _scenes import push_scene
    from simian_spacemonkey_amd import sortlast
    dims, nranks, halo, ring = (75, 21, 19), 2, 3, "u8"
    data, grad, wdata, wgrad, _, _ = reference(gpu_renderer_factory, kind, ring, dims)
    data2, grad2 = S.source(kind, ring, dims, seed=1)
    sc = T.scene(wdata, wgrad)
    opts = (("kernel", 1),)

    def run(side, other):
        rs = ranks_of(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), nranks, halo, opts=opts)
        try:
            for R in rs:
                push_scene(R, sc, upload=False)
            pd, k0 = dev(data2)
            pg, k1 = dev(grad2)
            keep = sortlast.stencil_timestep_local(rs, kind, 0, 1, stream=None if side is None else ctypes.c_void_p(side.cuda_stream))
            for R in rs:                                    # the source slot overwritten: behind the write pass's reads
                R.upload_timestep_device(0, pd, dims, data2.shape[-1], S.M.CODE[ring], pg, fsize=fsz(dims), dmode=dmode(kind, data2.shape[-1]),
                                         stream=None if other is None else ctypes.c_void_p(other.cuda_stream))
                R.select_timestep(1)
            lay, out = merged(rs, sc)
            downs = [R.download_timestep(1) for R in rs] + [R.download_timestep(0) for R in rs]
            del keep, k0, k1
            return lay, out, downs
        finally:
            close(rs)
    want = run(None, None)
    got = run(torch.cuda.Stream(), torch.cuda.Stream())
    assert want[1][..., 3].max() > 0.05
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    for (d0, g0), (d1, g1) in zip(want[2], got[2]):
        same(d1, d0, "a step made on the caller's stream")
        same(g1, g0, "its normals")
    g0r, g1r = S.stored_box(dims, 0, nranks, halo, ring)[:2]
    same(got[2][0][0], wdata[g0r[2]:g1r[2], g0r[1]:g1r[1], g0r[0]:g1r[0]], "rank 0's region")
    same(got[2][nranks][0], data2[g0r[2]:g1r[2], g0r[1]:g1r[1], g0r[0]:g1r[0]], "the new step 0")

