"""Time steps from a rank's own dense block of the volume (smk.h: smk_block, smk_declare_volume,
smk_upload_timestep_block_device, smk_block_extremes_device, smk_upload_timestep_scalar_block_device,
smk_upload_timestep_fields_block_device).  Expected values come from the EXISTING entries run in the same test on an
unsharded context that was given the whole arrays: smk_upload_volume, smk_upload_timestep_device,
smk_upload_timestep_scalar_device, smk_upload_timestep_fields_device and smk_step_extremes_device.  The cases are
tests/_step_shard_ref.py's, every rank's block in the three cuts of tests/_step_block_ref.py (qualified by
tests/test_step_block_cpu.py): volumes of a few ten thousand voxels."""
import ctypes

import numpy as np
import pytest

import _step_block_ref as B
import _step_shard_ref as S
import _tblend_ref as T
import _step_gpu as G
from _gpu_mem import dev_ptr as dev, fetch_layers, layer_buffer, merged, words_buf
from _step_gpu import (RAN, UndisturbedHalos as Undisturbed, arrays, close, declared, dmode, flags_of, fsz, hand_over, params, probe_at,
                       rank_context, ranks_declared, ranks_of, reference_of_arrays as reference, rim_tables, run_cut, same_bits as same,
                       uploaded_zeros)

pytestmark = pytest.mark.gpu
CODE = B.M.CODE
NP = B.M.NP


# ---- 1. the data-free geometry

@pytest.mark.parametrize("nranks", [1, 2])
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "none"])
@pytest.mark.parametrize("ring, nelts", [("u8", 3), ("u16", 3), ("f32", 3), ("f32", 4)])
def test_declare_volume_is_the_upload_of_zeros(gpu_renderer_factory, ring, nelts, normals, nranks):
    from _scenes import push_scene
    dims = (37, 13, 11)                                     # (odd x and y: a pad column and row of 8-byte voxels)
    dm = "VGH" if nelts == 3 else "V3G"
    sc = T.scene(np.zeros(dims[::-1] + (3,), NP[ring]), None)
    got = []
    for make in (uploaded_zeros, declared):
        R = make(gpu_renderer_factory, dims, ring, nelts, dm, nranks - 1, nranks, 3, normals, opts=(("kernel", 1),))
        try:
            push_scene(R, sc, upload=False)
            frame = R.render()
            cells = S.cells_of(*S.uploaded_valid(dims, *S.stored_box(dims, nranks - 1, nranks, 3, ring)[2:4]))
            got.append((R.download_timestep(), R.brick_flags(), R.timestep_box(), R.timestep_halo(), frame, R.timesteps(), R.probe_step(cells)))
        finally:
            R.close()
    (d0, g0), (d1, g1) = got[0][0], got[1][0]
    same(d1, d0, "data")
    same(g1, g0, "normals")
    assert not d0.any() and (g0 == 128).all()
    assert np.array_equal(got[1][1][0], got[0][1][0]) and got[1][1][1] == got[0][1][1]
    assert got[1][2] == got[0][2] and got[1][3] == got[0][3] == (3 if nranks > 1 else 1) and got[1][5] == got[0][5] == (0, [0])
    assert np.array_equal(got[1][4], got[0][4])
    for a, b in zip(got[1][6], got[0][6]):
        assert np.array_equal(a, b)
    assert got[0][6][2].all()


def test_declare_volume_refuses_what_an_upload_refuses(gpu_renderer_factory, smk):
    R = gpu_renderer_factory()
    try:
        for args, why in ((((8, 8, 8), 5, 0), "smk_declare_volume: nelts 5 not in 1..4"), (((8, 8, 8), 4, 2), "4-channel u16 voxels"),
                          (((8, 0, 8), 3, 0), "smk_declare_volume: brick 0 empty"), (((8, 8, 8), 3, 7), "smk_declare_volume: bad dtype")):
            with pytest.raises(smk.SmkError, match=why):
                R.declare_volume(args[0], args[1], args[2], fsize=(1., 1., 1.))
        with pytest.raises(smk.SmkError, match="smk_declare_volume: non-positive extent"):
            R.declare_volume((8, 8, 8), 3, 0, fsize=(1., 0., 1.))
        assert R.timesteps() == (-1, [])
        R.set_shard(1, 2)
        with pytest.raises(smk.SmkError, match="smk_declare_volume: volume too thin to shard"):
            R.declare_volume((8, 1, 8), 3, 0, fsize=(1., 1., 1.))
    finally:
        R.close()


# ---- 2. the packed form

@pytest.mark.parametrize("ring, nelts", [("u8", 3), ("u16", 2), ("f32", 3), ("f32", 4)])
def test_a_whole_volume_block_is_the_device_upload(gpu_renderer_factory, smk, ring, nelts):
    dims = (37, 13, 11)
    data, grad = T.step(ring, 1, dims, nelts)
    pd, k0 = dev(data)
    pg, k1 = dev(grad)
    dm = {2: "V1G", 3: "VGH", 4: "V3G"}[nelts]
    R = uploaded_zeros(gpu_renderer_factory, dims, ring, nelts, dm)
    try:
        R.upload_timestep_device(1, pd, dims, nelts, CODE[ring], pg, fsize=fsz(dims), dmode=dm)
        R.upload_timestep_block_device(2, pd, smk.smk_block((0, 0, 0), dims), pg)
        a, b = R.download_timestep(1), R.download_timestep(2)
        assert a[0].any() and R.timestep_halo(2) == R.timestep_halo(1) == 1 and R.timesteps() == (0, [0, 1, 2])
        same(b[0], a[0], "data")
        same(b[1], a[1], "normals")
        cells = S.cells_of((0, 0, 0), dims)
        for x, y in zip(R.probe_step(cells, 2), R.probe_step(cells, 1)):
            assert np.array_equal(x, y)
    finally:
        R.close()
    del k0, k1


PACKED = [pytest.param(i, ring, id="%s-%s" % (B.CASE_IDS[i], ring)) for i in range(len(B.CASES)) for ring in B.RINGS]


@pytest.mark.parametrize("which", B.CUTS)
@pytest.mark.parametrize("case, ring", PACKED)
def test_the_ranks_packed_blocks_assemble_to_the_uploaded_volume(gpu_renderer_factory, smk, case, ring, which):
    kind, dims, nranks, halo = B.CASES[case]
    data, grad = S.source(kind, ring, dims)
    U = rank_context(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]))
    try:
        wdata, wgrad = U.download_timestep(0)
        wprobe = U.probe_step(S.cells_of((0, 0, 0), dims), 0)
    finally:
        U.close()
    cuts = B.cuts_of(case, ring, which, reach=0)
    rs = ranks_declared(gpu_renderer_factory, dims, ring, data.shape[-1], dmode(kind, data.shape[-1]), cuts)
    parts, gparts, keep = [], [], []
    try:
        for R, c in zip(rs, cuts):
            pd, k0, blk = hand_over(smk, c, data, ring)
            pg, k1, _ = hand_over(smk, c, grad, "u8")
            keep += [k0, k1]
            R.upload_timestep_block_device(1, pd, blk, pg)
            assert R.timestep_halo(1) == c.halo == c.src_halo and R.timesteps() == (0, [0, 1])
            origin, size, ne, dt, hn = R.timestep_box()
            got = R.download_timestep(1)
            parts.append((origin, got[0]))
            gparts.append((origin, got[1]))
            cells = S.cells_of(c.stored_lo, c.stored_hi)
            raw, nrm, ok = R.probe_step(cells, 1)
            inside = np.all((cells >= np.array(c.lo)) & (cells + 1 < np.array(c.hi)), -1)
            assert np.array_equal(ok, inside), "rank %d: %d cells answered, %d lie in C" % (c.rank, ok.sum(), inside.sum())
            wraw, wnrm = probe_at(wprobe, dims, cells[inside])
            same(raw[inside], wraw, "rank %d: C's voxels" % c.rank)
            same(nrm[inside], wnrm, "rank %d: C's normals" % c.rank)
            # (an unanswered cell comes back as zeros from the host: that says nothing of the rim, which
            # test_the_rim_is_zeros_over_what_the_slot_held looks at)
            assert not raw[~inside].any() and not nrm[~inside].any()
        del keep
    finally:
        close(rs)
    same(S.place(dims, wdata.shape[-1], wdata.dtype, parts), wdata, "data")
    same(S.place(dims, 3, np.uint8, gparts), wgrad, "normals")


# ---- 3. the words, 4. the voxels

def check_cut(rs, cuts, kind, dims, out, words, ref):
    arr, wdata, wgrad, wprobe, wwords = ref
    nranks = len(rs)
    w = words.cpu().numpy()
    assert np.array_equal(w[nranks], wwords), (w, wwords)
    assert np.array_equal(B.combine(w[:nranks]), wwords)
    parts, gparts = [], []
    for R, c in zip(rs, cuts):
        inner = S.has_interior(dims, c.g0, c.g1)
        assert np.array_equal(w[c.rank], B.SEEDS[kind]) == (not inner), "rank %d: seed-only words exactly without an interior voxel" % c.rank
        if kind == "derive":                                # the V words are the region's own, whatever the block holds beyond it
            assert np.array_equal(w[c.rank][:2], B.region_words(kind, arr[0][..., None], c.g0, c.g1)[:2]), (c.which, c.rank)
        origin, size, ne, dt, hn = R.timestep_box()
        assert origin == c.g0
        got = R.download_timestep(out)
        parts.append((origin, got[0]))
        gparts.append((origin, got[1]))
        assert R.timestep_halo(out) == c.halo, (c.which, c.rank, R.timestep_halo(out), c.halo)
        cells = S.cells_of(c.stored_lo, c.stored_hi)
        raw, nrm, ok = R.probe_step(cells, out)
        inside = np.all((cells >= np.array(c.vlo)) & (cells + 1 < np.array(c.vhi)), -1)
        assert np.array_equal(ok, inside), "cut %s rank %d: %d cells answered, %d lie in the valid box" % (c.which, c.rank, ok.sum(), inside.sum())
        assert (S.straddles(cells, c.g0, c.g1) & inside).any()
        wraw, wnrm = probe_at(wprobe, dims, cells[inside])
        same(raw[inside], wraw, "cut %s rank %d: the valid box's voxels" % (c.which, c.rank))
        same(nrm[inside], wnrm, "cut %s rank %d: the valid box's normals" % (c.which, c.rank))
        assert not raw[~inside].any() and not nrm[~inside].any()     # (unanswered cells are zeroed on the host; the rim: section 4b)
    same(S.place(dims, wdata.shape[-1], wdata.dtype, parts), wdata, "data")
    same(S.place(dims, 3, np.uint8, gparts), wgrad, "normals")


def check_case(factory, smk, kind, ring, case, sd=None, nf=2, compat=1, blur=0, normals=True, which=B.CUTS):
    _, dims, nranks, halo = B.CASES[case]
    sd = sd or ring
    ref = reference(factory, kind, ring, dims, sd, nf, compat, blur, normals)
    nelts = 3 if kind == "derive" else nf + 1
    for group in (("a", "b"), ("c",)):                      # (a) and (b) share option halo, and so their contexts
        group = [wc for wc in group if wc in which]
        if not group:
            continue
        cuts = [B.cuts_of(case, ring, wc) for wc in group]
        rs = ranks_declared(factory, dims, ring, nelts, dmode(kind, nelts), cuts[0], normals)
        try:
            for out, cs in enumerate(cuts, 1):
                keep, words = run_cut(smk, rs, cs, kind, ring, sd, ref[0], out, compat, blur)
                check_cut(rs, cs, kind, dims, out, words, ref)
                del keep
        finally:
            close(rs)
    if not normals:
        assert (ref[2] == 128).all()


CASES = [pytest.param(i, ring, id="%s-%s" % (B.CASE_IDS[i], ring)) for i in range(len(B.CASES)) for ring in B.RINGS]


@pytest.mark.parametrize("case, ring", CASES)
def test_the_ranks_blocks_give_the_unsharded_step(gpu_renderer_factory, smk, case, ring):
    kind = B.CASES[case][0]
    compat, blur = params(kind, case)
    check_case(gpu_renderer_factory, smk, kind, ring, case, compat=compat, blur=blur)


@pytest.mark.parametrize("n, sd, ring", [(n, sd, ring) for n, (sd, ring) in enumerate((sd, ring) for sd in B.RINGS for ring in B.RINGS) if sd != ring])
def test_a_scalar_of_any_type_into_a_ring_of_any_type(gpu_renderer_factory, smk, n, sd, ring):
    compat, blur = params("derive", n)
    check_case(gpu_renderer_factory, smk, "derive", ring, 0, sd=sd, compat=compat, blur=blur)


@pytest.mark.parametrize("ring, nf", [("u8", 1), ("u8", 3), ("u16", 1), ("f32", 1), ("f32", 3)])
def test_merge_of_one_to_three_fields(gpu_renderer_factory, smk, ring, nf):
    check_case(gpu_renderer_factory, smk, "merge", ring, 6, nf=nf)


@pytest.mark.parametrize("kind, ring, nf, case", [("derive", "u8", 2, 0), ("derive", "f32", 2, 0), ("merge", "u16", 2, 7), ("merge", "f32", 3, 7)])
def test_a_context_without_normals(gpu_renderer_factory, smk, kind, ring, nf, case):
    check_case(gpu_renderer_factory, smk, kind, ring, case, nf=nf, normals=False)


@pytest.mark.parametrize("kind, ring, sd, nf", [("derive", "u8", "u8", 2), ("derive", "u16", "f32", 2), ("derive", "f32", "u16", 2), ("merge", "u8", "u8", 3),
                                                 ("merge", "u16", "u16", 2), ("merge", "f32", "f32", 3)])
def test_extremes_and_write_on_an_unsharded_context_is_the_one_call_entry(gpu_renderer_factory, smk, kind, ring, sd, nf):
    dims = (37, 13, 11)
    arr, wdata, wgrad, _, wwords = reference(gpu_renderer_factory, kind, ring, dims, sd, nf, 1, 1)
    nelts = 3 if kind == "derive" else nf + 1
    held = [dev(a) for a in arr]
    ptrs = [h[0] for h in held]
    blk = smk.smk_block((0, 0, 0), dims)
    R = declared(gpu_renderer_factory, dims, ring, nelts, dmode(kind, nelts))
    try:
        w = words_buf()
        R.block_extremes_device(0 if kind == "derive" else 1, ptrs, CODE[sd], blk, w.data_ptr())
        if kind == "derive":
            R.upload_timestep_scalar_block_device(1, ptrs[0], CODE[sd], blk, w.data_ptr(), 1, 1)
        else:
            R.upload_timestep_fields_block_device(1, ptrs, CODE[sd], blk, w.data_ptr())
        got = R.download_timestep(1)
        assert np.array_equal(w.cpu().numpy()[0], wwords) and R.timestep_halo(1) == 1
    finally:
        R.close()
    same(got[0], wdata, "data")
    same(got[1], wgrad, "normals")


# ---- 4b. the rim, seen.  Nothing reads a stored voxel outside a step's valid box back: the probe answers inside it only, the
# read-back gives the region.  The brick summaries are made over the WHOLE stored box, and the brick flags show them: under
# a table that is transparent at the lowest few values alone a brick of rim voxels is flagged when one of them is not near zero, and
# under a table that is opaque at the top values alone every brick that touches a rim of stale top values is flagged.

@pytest.mark.parametrize("form", ["packed", "derive", "merge"])
def test_the_rim_is_zeros_over_what_the_slot_held(gpu_renderer_factory, smk, form):
    """A step of top values everywhere goes up through an existing entry; the same id is overwritten in place by a block form
    whose rim is not empty; the flags must be those of a context that UPLOADED the result with its rim zeroed, and differ from
    those of one that uploaded it with the top values left on the rim.  Rank 0's stored box ends on a brick of rim voxels
    alone (77 voxels in x: a region of 38, stored to 42 or 44, the last brick from voxel 40), which the first table sees."""
    import torch
    dims, nranks, ring, halo = (77, 21, 19), 2, "u8", 3
    kind = "merge" if form == "merge" else "derive"
    if form == "packed":                                    # region +- 1 under a larger option halo: a rim of 4 voxels and the evening's
        arr, (wdata, wgrad), words = None, S.source(kind, ring, dims), None
        cuts = [B.Cut(kind, dims, r, nranks, halo, ring, "c", reach=0) for r in range(nranks)]
    else:                                                   # cut (a): the reach's rim and the evening's voxel
        arr, wdata, wgrad, _, words = reference(gpu_renderer_factory, kind, ring, dims)
        cuts = [B.Cut(kind, dims, r, nranks, halo, ring, "a") for r in range(nranks)]
        words = torch.tensor(words, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()                            # the words are on the device before a context's stream reads them
    nz, ny, nx = dims[::-1]
    stale = np.full((nz, ny, nx, 3), 255, np.uint8)
    sgrad = np.full((nz, ny, nx, 3), 7, np.uint8)
    sc = T.scene(wdata, wgrad)
    opts = (("kernel", 1),)
    seen = [False, False]
    for c in cuts:
        outside = ~S.in_box((nz, ny, nx), (0, 0, 0), c.vlo, c.vhi)
        assert outside[c.stored_lo[2]:c.stored_hi[2], c.stored_lo[1]:c.stored_hi[1], c.stored_lo[0]:c.stored_hi[0]].any(), "a rim"
        want = []
        for fill, gfill in ((0, 128), (255, 7)):            # the result with its rim zeroed; with the stale step left on it
            d, g = wdata.copy(), wgrad.copy()
            d[outside], g[outside] = fill, gfill
            U = rank_context(gpu_renderer_factory, dims, d, g, dmode(kind, d.shape[-1]), c.rank, nranks, c.option_halo, opts=opts)
            try:
                want.append(flags_of(U, sc, 0, rim_tables()))
            finally:
                U.close()
        R = rank_context(gpu_renderer_factory, dims, stale, sgrad, dmode(kind, stale.shape[-1]), c.rank, nranks, c.option_halo, cap=3, opts=opts)
        try:
            R.upload_timestep(1, stale, sgrad, fsize=fsz(dims), dmode=dmode(kind, 3))
            before = flags_of(R, sc, 1, rim_tables())
            if form == "packed":
                pd, k0, blk = hand_over(smk, c, wdata, ring)
                pg, k1, _ = hand_over(smk, c, wgrad, "u8")
                R.upload_timestep_block_device(1, pd, blk, pg)
            else:
                held = [hand_over(smk, c, a, ring) for a in arr]
                ptrs, blk = [h[0] for h in held], held[0][2]
                if form == "derive":
                    R.upload_timestep_scalar_block_device(1, ptrs[0], CODE[ring], blk, words.data_ptr(), 1, 0)
                else:
                    R.upload_timestep_fields_block_device(1, ptrs, CODE[ring], blk, words.data_ptr())
            assert R.timesteps() == (1, [0, 1]) and R.timestep_halo(1) == c.halo      # (the shown step, overwritten in place)
            got = flags_of(R, sc, 1, rim_tables())
        finally:
            R.close()
        assert before[0].all() and before[1].all(), "the stale step flags every brick under both tables"
        for t in (0, 1):
            assert np.array_equal(got[t], want[0][t]), "rank %d, table %d: %d bricks differ from the zeroed rim's" % (
                c.rank, t, (got[t] != want[0][t]).sum())
            seen[t] |= not np.array_equal(want[1][t], want[0][t])
        assert not np.array_equal(want[1][1], want[0][1]), "rank %d: the second table tells a stale rim from a zeroed one" % c.rank
    assert all(seen), "both tables tell a stale rim from a zeroed one on some rank: %s" % seen


# ---- 5. frames

@pytest.mark.parametrize("bricks", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2], ids=["gather", "slice-ring"])
@pytest.mark.parametrize("kind, ring, case, which", [("derive", "u8", 0, "a"), ("derive", "f32", 0, "c"), ("merge", "u16", 7, "b")])
def test_frames_of_the_produced_step(gpu_renderer_factory, smk, kind, ring, case, which, kernel, bricks):
    from _scenes import push_scene
    _, dims, nranks, halo = B.CASES[case]
    if nranks > 2:
        nranks = 2
    cuts = [B.Cut(kind, dims, r, nranks, halo, ring, which) for r in range(nranks)]
    arr, wdata, wgrad, _, _ = reference(gpu_renderer_factory, kind, ring, dims)
    opts = (("kernel", kernel), ("bricks", bricks), ("slab_split", 1))
    sc = T.scene(wdata, wgrad)

    def frames(rs):
        for R in rs:
            push_scene(R, sc, upload=False)
        lay, out = merged(rs, sc)
        assert all(R.last_frame_info()[0] == RAN[kernel] for R in rs) and all(R.stat("slab_failures") == 0 for R in rs)
        return lay, out
    up = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, dmode(kind, wdata.shape[-1]), nranks, cuts[0].option_halo, opts=opts)     # ... that UPLOADED the unsharded result
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
    rs = ranks_declared(gpu_renderer_factory, dims, ring, 3, dmode(kind, 3), cuts, opts=opts)
    try:
        frames(rs)                                          # (the declared zeros rendered first: flags and plans of another step exist)
        keep = run_cut(smk, rs, cuts, kind, ring, ring, arr, 1, 1, 0)
        for R in rs:
            R.select_timestep(1)
        got_layers, got = frames(rs)
        del keep
    finally:
        close(rs)
    assert whole[..., 3].max() > 0.05 and all(l[..., 3].max() > 0.01 for l in want_layers)
    err = np.abs(got - whole).max()
    assert err <= G.SORT_LAST_TOL, "merged against the unsharded frame: max abs err %g" % err
    for r in range(nranks):                                 # (a rim is never sampled: the layers are those of the uploaded result)
        assert np.array_equal(got_layers[r], want_layers[r]), "rank %d: max diff %g" % (r, np.abs(got_layers[r] - want_layers[r]).max())
    assert np.array_equal(got, want)


# ---- 6. refusals

@pytest.mark.parametrize("kind", ["derive", "merge"])
def test_refusals_leave_the_ring_unchanged(gpu_renderer_factory, smk, kind):
    from _scenes import push_scene
    dims, nranks = (37, 13, 11), 2
    reach = B.REACH[kind]
    code = 0 if kind == "derive" else 1
    ring = "u8"
    entry = "smk_upload_timestep_%s_block_device" % ("scalar" if kind == "derive" else "fields")
    data, grad = S.source(kind, ring, dims)
    sc = T.scene(data, grad)
    arr = arrays(kind, ring, dims, ring, 2)
    held = [dev(a) for a in arr]
    ptrs = [h[0] for h in held]
    pd, k0 = dev(data)
    pg, k1 = dev(grad)
    w = words_buf()
    p = w.data_ptr()
    whole = smk.smk_block((0, 0, 0), dims)

    def write(R, t, ptrs_, dt, blk, pw):
        if kind == "derive":
            R.upload_timestep_scalar_block_device(t, None if ptrs_ is None else ptrs_[0], dt, blk, pw)
        else:
            R.upload_timestep_fields_block_device(t, ptrs_, dt, blk, pw)
    R = gpu_renderer_factory()
    try:
        for call, who in ((lambda: write(R, 1, ptrs, 0, whole, p), entry), (lambda: R.block_extremes_device(code, ptrs, 0, whole, p), "smk_block_extremes_device"),
                          (lambda: R.upload_timestep_block_device(1, pd, whole, pg), "smk_upload_timestep_block_device")):
            with pytest.raises(smk.SmkError, match=who + ": no volume"):
                call()
    finally:
        R.close()
    halo = reach + 1
    g0, g1, O, D, pad = S.stored_box(dims, 0, nranks, halo, ring)           # rank 0: x [0, 18), stored to 18 + halo (evened)
    R = rank_context(gpu_renderer_factory, dims, data, grad, dmode(kind, data.shape[-1]), 0, nranks, halo, cap=2, opts=(("kernel", 1),))
    try:
        push_scene(R, sc, upload=False)
        R.upload_timestep(1, data, grad, fsize=fsz(dims), dmode=dmode(kind, 3))
        blk = lambda o, s, py=0, pz=0: smk.smk_block(o, s, py, pz)      # noqa: E731
        ok = blk((0, 0, 0), dims)
        short = blk((0, 0, 0), (g1[0] + reach, dims[1], dims[2]))          # a valid halo of `reach`
        with Undisturbed(R):
            for b, why in ((None, "block is NULL"), (blk((0, 0, 0), (dims[0], 0, dims[2])), "sizes are > 0"),
                           (blk((0, 0, 0), dims, dims[0] - 1), r"pitch_y %d is below the block's %d voxels per row" % (dims[0] - 1, dims[0])),
                           (blk((0, 0, 0), dims, dims[0], dims[0] * dims[1] - 1), "pitch_z %d is below" % (dims[0] * dims[1] - 1)),
                           (blk((1, 0, 0), dims), r"the block \[1, 38\) of axis x lies outside the volume 37x13x11"),
                           (blk((0, -1, 0), dims), r"the block \[-1, 12\) of axis y lies outside the volume"),
                           (blk((1, 0, 0), (dims[0] - 1, dims[1], dims[2])), r"holds voxels \[1, %d\) of axis x .* its region is \[0, %d\)" % (O[0] + D[0], g1[0])),
                           (blk((0, 0, 0), (g1[0] - 1, dims[1], dims[2])), r"holds voxels \[0, %d\) of axis x .* its region is \[0, %d\)" % (g1[0] - 1, g1[0]))):
                for call in (lambda: write(R, 5, ptrs, 0, b, p), lambda: R.block_extremes_device(code, ptrs, 0, b, p),
                             lambda: R.upload_timestep_block_device(5, pd, b, pg)):
                    with pytest.raises(smk.SmkError, match=why):
                        call()
            for call in (lambda: write(R, 5, ptrs, 0, short, p), lambda: R.block_extremes_device(code, ptrs, 0, short, p)):
                with pytest.raises(smk.SmkError, match=r"the block gives a valid halo of %d voxels, the stencil reaches %d .*>= %d is needed" % (reach, reach, reach + 1)):
                    call()
            with pytest.raises(smk.SmkError, match=r"smk_upload_timestep_block_device: the block gives a valid halo of 0 voxels"):
                R.upload_timestep_block_device(5, pd, blk((0, 0, 0), (g1[0], dims[1], dims[2])), pg)
            for call, why in (
                    (lambda: write(R, -1, ptrs, 0, ok, p), entry + ": time step -1: ids are >= 0"),
                    (lambda: write(R, 5, ptrs, 0, ok, None), "d_words is NULL"),
                    (lambda: write(R, 5, ptrs, 0, ok, p + 2), "d_words is not aligned"),
                    (lambda: write(R, 5, None, 0, ok, p), "d_scalar is NULL" if kind == "derive" else "d_fields is NULL"),
                    (lambda: write(R, 5, ptrs, 7 if kind == "derive" else 1, ok, p),
                     "scalar_dtype 7 is none of" if kind == "derive" else "field_dtype 1 is not the ring's type"),
                    (lambda: R.block_extremes_device(7, ptrs, 0, ok, p), "smk_block_extremes_device: kind 7 is neither"),
                    (lambda: R.block_extremes_device(code, ptrs, 0, ok, None), "d_words is NULL"),
                    (lambda: R.block_extremes_device(code, ptrs + ptrs, 0, ok, p), "the derive takes one scalar" if kind == "derive" else "4 fields for a series of nelts 3"),
                    (lambda: R.upload_timestep_block_device(-1, pd, ok, pg), "smk_upload_timestep_block_device: time step -1: ids are >= 0"),
                    (lambda: R.upload_timestep_block_device(5, None, ok, pg), "d_data is NULL"),
                    (lambda: R.upload_timestep_block_device(5, pd, ok, None), "normals absent, the series' present"),
                    ):
                with pytest.raises(smk.SmkError, match=why):
                    call()
            if kind == "merge":
                with pytest.raises(smk.SmkError, match=r"d_fields\[1\] is NULL"):
                    write(R, 5, [ptrs[0], None], 0, ok, p)
        assert (w.cpu().numpy() == 0x5a5a5a5a).all(), "a refused export writes no word"
    finally:
        R.close()
    # no slot: a ring of one step, the current one
    one = declared(gpu_renderer_factory, dims, ring, 3, dmode(kind, 3), cap=1)
    try:
        for call, who in ((lambda: write(one, 5, ptrs, 0, whole, p), entry), (lambda: one.upload_timestep_block_device(5, pd, whole, pg), "smk_upload_timestep_block_device")):
            with pytest.raises(smk.SmkError, match=who + r": time step 5: the cache holds one step, the current one \(0\)"):
                call()
        assert one.timesteps() == (0, [0]) and not one.download_timestep(0)[0].any()
    finally:
        one.close()
    # a misaligned array, and the nelts rules
    f32 = declared(gpu_renderer_factory, dims, "f32", 3, dmode(kind, 3), cap=3)
    try:
        with pytest.raises(smk.SmkError, match="is not aligned to its 4-byte elements"):
            write(f32, 1, [q + 2 for q in ptrs], 1, whole, p)
        assert f32.timesteps() == (0, [0])
    finally:
        f32.close()
    ne = 2 if kind == "derive" else 1
    R = declared(gpu_renderer_factory, dims, ring, ne, "V1G" if ne == 2 else "V1", 0, nranks, 3, cap=3)
    try:
        why = "nelts 2: V, G and H are three channels" if kind == "derive" else "nelts 1: a multi-field step is at least one field and G"
        for call in (lambda: write(R, 1, ptrs, 0, whole, p), lambda: R.block_extremes_device(code, ptrs, 0, whole, p)):
            with pytest.raises(smk.SmkError, match=why):
                call()
        assert R.timesteps() == (0, [0])
    finally:
        R.close()
    del k0, k1, held


# ---- 7. streams

@pytest.mark.parametrize("kind", ["derive", "merge"])
def test_on_a_stream_of_the_callers(gpu_renderer_factory, smk, kind):
    """export, combine, write and the frames on one non-default stream with no host wait between them: the bits are those of
    the contexts' own streams with the combine's two waits"""
    import torch
    from _scenes import push_scene
    case, ring = (0, "u8") if kind == "derive" else (6, "u16")
    _, dims, nranks, halo = B.CASES[case]
    cuts = B.cuts_of(case, ring, "b")
    arr, wdata, wgrad, _, _ = reference(gpu_renderer_factory, kind, ring, dims)
    sc = T.scene(wdata, wgrad)

    def run(side):
        st = None if side is None else ctypes.c_void_p(side.cuda_stream)
        rs = ranks_declared(gpu_renderer_factory, dims, ring, 3, dmode(kind, 3), cuts, opts=(("kernel", 1),))
        try:
            for R in rs:
                push_scene(R, sc, upload=False)
            layers = layer_buffer(rs, sc)
            keep = run_cut(smk, rs, cuts, kind, ring, ring, arr, 1, 1, 0, stream=st)
            for r, R in enumerate(rs):
                R.select_timestep(1)
                R.render_device(layers[r].data_ptr(), None, st)
            lay = fetch_layers(layers, sc)
            downs = [R.download_timestep(1) for R in rs]
            del keep
            return lay, downs
        finally:
            close(rs)
    want = run(None)
    got = run(torch.cuda.Stream())
    assert want[0][..., 3].max() > 0.01
    assert np.array_equal(got[0], want[0])
    for (d0, g0), (d1, g1), c in zip(want[1], got[1], cuts):
        same(d1, d0, "a step made on the caller's stream")
        same(g1, g0, "its normals")
        same(d1, wdata[c.g0[2]:c.g1[2], c.g0[1]:c.g1[1], c.g0[0]:c.g1[0]], "rank %d's region" % c.rank)
