"""Chains of step producers on sharded contexts (smk.h: "A source that has a rim itself (a second stencil) shrinks from its own
valid box"; a block step's valid box and valid halo, which "every later producer" respects): packed blocks, block stencils,
uploads and blends feeding smk_step_extremes_device + smk_derive_timestep_shard / smk_merge_timestep_shard.  Expected values
come from the SAME chain through the existing one-call entries on one unsharded context that was given the whole arrays
(smk_upload_timestep_device, smk_blend_timesteps, smk_derive_timestep, smk_merge_timestep, smk_upload_timestep_scalar_device,
smk_upload_timestep_fields_device), made once per case and shared: every rank's valid box, halo, words, region and histogram
must be that context's, bit for bit.  What is valid comes from the mask model of tests/_step_chain_ref.py (qualified by
tests/test_step_chain_cpu.py); the volumes are a few thousand voxels.

The witness (section 3) shows that the data can tell a voxel fed by the source's rim from an exact one: on every rank with a
telling face -- the stored box ends on the volume's face, the source's valid box inside the volume -- a source zeroed outside
what the rank holds valid gives, on an unsharded context and under the true words, the true bits on the model's box and other
bits in the layers between the source's box and the model's.  A valid box that is the reach too large there cannot pass."""
import numpy as np
import pytest

import _step_block_ref as B
import _step_chain_ref as C
import _step_read_ref as D
import _step_shard_ref as S
import _tblend_ref as T
import _step_gpu as G
from _gpu_mem import dev_ptr as dev, merged, words_buf
from _step_gpu import (RAN, UndisturbedHalos as Undisturbed, close, declared, dmode, export, flags_of, fsz, one_call, probe_at, rank_context,
                       ranks_declared, ranks_of, rim_tables, same_bits as same, write_shard)

pytestmark = pytest.mark.gpu
CODE = B.M.CODE
CAP = 6                                                     # step 0 (the declared zeros) and the chain's steps


def params(case):
    """(compat, blur) of the derive in case `case`: both flags take both values over the case list"""
    return ((1, 0), (0, 1), (1, 1), (0, 0))[case % 4]


def sources(ring, dims):
    """{seed: (data [z][y][x][3], normals)} of the two steps the chains read, and the dense fields of seed 0"""
    src = {seed: S.source("merge", ring, dims, 2, seed) for seed in (0, 1)}
    F = B.M.fields(ring, 2, dims, 0)
    return src, [np.ascontiguousarray(F[..., e]) for e in range(2)]


def dense(kind, ring, dims, fields):
    return [B.scalar(ring, dims)] if kind == "derive" else fields


def dmode_of(links):
    return dmode(C.final_kind(links), 3)


# ---- the unsharded chain

_REF = {}


class Ref:
    """the chain on an unsharded context: per step its (data, normals) and probe of every cell of the volume, per sharded
    stencil link the words that context exports for the link's source, and the final step's histogram"""


def unsharded_link(U, link, src, fields, dims, ring, dm, compat, blur, keep):
    what, out = link[0], link[1]
    if what in ("upload", "block"):
        data, grad = src[link[2]]
        (pd, k0), (pg, k1) = dev(data), dev(grad)
        keep += [k0, k1]
        U.upload_timestep_device(out, pd, dims, 3, CODE[ring], pg, fsize=fsz(dims), dmode=dm)
    elif what == "block_stencil":
        held = [dev(a) for a in dense(link[2], ring, dims, fields)]
        keep += held
        if link[2] == "derive":
            U.upload_timestep_scalar_device(out, held[0][0], CODE[ring], dims, compat, blur)
        else:
            U.upload_timestep_fields_device(out, [h[0] for h in held], CODE[ring], dims)
    elif what == "blend":
        U.blend_timesteps(link[2], link[3], link[4], out)
    else:
        one_call(U, link[2], link[3], out, compat, blur)


def reference_of(factory, cid, dims, links, ring, compat, blur):
    k = (cid, ring)
    if k not in _REF:
        src, fields = sources(ring, dims)
        dm = dmode_of(links)
        ref = Ref()
        ref.steps, ref.probe, ref.words, keep = {}, {}, {}, []
        cells = S.cells_of((0, 0, 0), dims)
        U = declared(factory, dims, ring, 3, dm, cap=CAP)
        try:
            for link in links:
                if link[0] == "stencil":
                    ref.words[link[1]] = export(U, link[2], link[3], compat)
                unsharded_link(U, link, src, fields, dims, ring, dm, compat, blur, keep)
                ref.steps[link[1]] = U.download_timestep(link[1])
                ref.probe[link[1]] = U.probe_step(cells, link[1])
                assert ref.probe[link[1]][2].all() and ref.steps[link[1]][0].any()
            ref.hist = U.hist2d_step(C.final(links))
        finally:
            U.close()
        del keep
        for d, g in ref.steps.values():
            d.setflags(write=False)
            g.setflags(write=False)
        _REF[k] = ref
    return _REF[k]


def reference(factory, case, ring):
    cid, dims, nranks, halo, links = C.CASES[case]
    return reference_of(factory, cid, dims, links, ring, *params(case))


def exact(got, want, cells, what):
    """probe answers [n][8][c] against the unsharded chain's, bit for bit; the first voxel that differs is named"""
    g, w = D.bits(got), D.bits(want)
    assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
    bad = np.argwhere(g != w)
    if len(bad):
        n, corner, ch = (int(v) for v in bad[0])
        x, y, z = (int(v) for v in cells[n] + np.array([corner & 1, (corner >> 1) & 1, corner >> 2]))
        raise AssertionError("%s: %d values in %d cells differ, first at voxel x %d y %d z %d channel %d: got %#x, the unsharded chain has %#x" % (
            what, len(bad), len(np.unique(bad[:, 0])), x, y, z, ch, int(g[n, corner, ch]), int(w[n, corner, ch])))


# ---- the chain on the ranks

def declared_ranks(factory, ranks, dm, opts=(), cap=CAP):
    return ranks_declared(factory, ranks[0].dims, ranks[0].ring, 3, dm, ranks, cap=cap, opts=opts)


def sharded_link(smk, rs, ranks, link, src, fields, dm, compat, blur, keep):
    """one link on every rank; the words tensor of a stencil link ([P + 1][8], row P combined), else None"""
    from simian_spacemonkey_amd import sortlast
    what, out = link[0], link[1]
    dims, ring = ranks[0].dims, ranks[0].ring
    if what == "upload":
        data, grad = src[link[2]]
        for R in rs:
            R.upload_timestep(out, data, grad, fsize=fsz(dims), dmode=dm)
    elif what == "block":
        data, grad = src[link[2]]
        for R, K in zip(rs, ranks):
            b = K.block(link[3])
            (pd, k0), (pg, k1) = dev(b.take(data)), dev(b.take(grad))
            keep += [k0, k1]
            R.upload_timestep_block_device(out, pd, smk.smk_block(b.origin, b.size), pg)
    elif what == "block_stencil":
        blocks = []
        for K in ranks:
            b = K.block(link[3])
            held = [dev(b.take(a)) for a in dense(link[2], ring, dims, fields)]
            keep += held
            blocks.append(([h[0] for h in held], CODE[ring], smk.smk_block(b.origin, b.size)))
        return sortlast.stencil_block_local(rs, link[2], blocks, out, compat=compat, blur=blur)
    elif what == "blend":
        for R in rs:
            R.blend_timesteps(link[2], link[3], link[4], out)
    else:
        return sortlast.stencil_timestep_local(rs, link[2], link[3], out, compat=compat, blur=blur)
    return None


def run_chain(smk, rs, ranks, links, ring, compat, blur):
    """the whole chain on the ranks: ({out of a stencil link: words [P + 1][8]}, what keeps the blocks alive)"""
    src, fields = sources(ring, ranks[0].dims)
    dm, keep, words = dmode_of(links), [], {}
    for link in links:
        w = sharded_link(smk, rs, ranks, link, src, fields, dm, compat, blur, keep)
        if w is not None:
            words[link[1]] = w
    return words, keep


CASES = [pytest.param(i, ring, id="%s-%s" % (C.CASE_IDS[i], ring)) for i in range(len(C.CASES)) for ring in C.RINGS]


# ---- 1. the valid box, the halo, the words, the regions and the histogram of every step of every chain

@pytest.mark.parametrize("case, ring", CASES)
def test_every_step_of_the_chain_is_the_unsharded_chains(gpu_renderer_factory, smk, case, ring):
    cid, dims, nranks, halo, links = C.CASES[case]
    compat, blur = params(case)
    ref = reference(gpu_renderer_factory, case, ring)
    ranks = C.ranks_of(case, ring)
    model = [C.run(K, links) for K in ranks]
    rs = declared_ranks(gpu_renderer_factory, ranks, dmode_of(links))
    n_cells = n_rim = 0
    try:
        words, keep = run_chain(smk, rs, ranks, links, ring, compat, blur)
        for out, w in words.items():
            if out in ref.words:
                assert np.array_equal(w.cpu().numpy()[nranks], ref.words[out]), "step %d: the combined words %s, the unsharded export %s" % (
                    out, w.cpu().numpy()[nranks], ref.words[out])
        hist = np.zeros((256, 256), np.int64)
        parts = {link[1]: ([], []) for link in links}
        for R, K, steps in zip(rs, ranks, model):
            assert R.timesteps()[1] == [0] + [link[1] for link in links]
            origin = R.timestep_box()[0]
            assert origin == K.g0
            cells = S.cells_of(K.stored_lo, K.stored_hi)
            for link in links:
                out, st = link[1], steps[link[1]]
                who = "%s rank %d step %d (%s)" % (cid, K.rank, out, link[0])
                assert R.timestep_halo(out) == st.halo, "%s: valid halo %d, the model's %d" % (who, R.timestep_halo(out), st.halo)
                lo, hi = st.box
                raw, nrm, ok = R.probe_step(cells, out)
                inside = np.all((cells >= np.array(lo)) & (cells + 1 < np.array(hi)), -1)
                assert inside.any()
                # what is answered is exact (a voxel computed from the source's rim is not) ...
                araw, anrm = probe_at(ref.probe[out], dims, cells[ok])
                exact(raw[ok], araw, cells[ok], who + ": the answered cells' voxels")
                exact(nrm[ok], anrm, cells[ok], who + ": the answered cells' normals")
                # ... and the answered cells are those of the model's box
                bad = np.argwhere(ok != inside)
                assert not len(bad), "%s: %d cells answered, %d lie in the model's box %s..%s; first other cell %s (answered: %s)" % (
                    who, ok.sum(), inside.sum(), lo, hi, tuple(cells[bad[0][0]]), bool(ok[bad[0][0]]))
                wraw, wnrm = probe_at(ref.probe[out], dims, cells[inside])
                same(raw[inside], wraw, who + ": the valid box's voxels")
                same(nrm[inside], wnrm, who + ": the valid box's normals")
                assert not raw[~inside].any() and not nrm[~inside].any(), who + ": an unanswered cell is zeros"
                got = R.download_timestep(out)
                parts[out][0].append((origin, got[0]))
                parts[out][1].append((origin, got[1]))
                if out == C.final(links):
                    n_cells += int(inside.sum())
                    n_rim += int((K.stored() & ~st.mask).sum())
            hist += R.hist2d_step(C.final(links))
        del keep, words
    finally:
        close(rs)
    for link in links:
        wdata, wgrad = ref.steps[link[1]]
        same(S.place(dims, 3, wdata.dtype, parts[link[1]][0]), wdata, "step %d: the regions' data" % link[1])
        same(S.place(dims, 3, np.uint8, parts[link[1]][1]), wgrad, "step %d: the regions' normals" % link[1])
    same(hist.astype(ref.hist.dtype), ref.hist, "the ranks' histograms of the final step, summed")
    print("CHAIN %s %s: %d cells compared inside the final valid boxes, %d rim voxels" % (cid, ring, n_cells, n_rim))


# ---- 2. the rim after the last stencil: zeros over what the slot held (the tables of tests/test_gpu_step_block.py, 4b)

RIM = {"merge": ((24, 9, 13), 2, 12, C.chain_a("merge")), "derive": ((24, 9, 13), 2, 12, C.chain_a("derive"))}


@pytest.mark.parametrize("kind", ["merge", "derive"])
def test_the_rim_of_the_last_stencil_is_zeros_over_what_the_slot_held(gpu_renderer_factory, smk, kind):
    """24 voxels in x under option halo 12: both ranks store all of x, their blocks reach 2 or 3 voxels beyond the region, so
    the result's rim holds the whole brick of x 16..23 (rank 0) and 0..7 (rank 1), which the first table sees.  The final id
    held a step of top values before the chain overwrote it in place."""
    dims, nranks, halo, links = RIM[kind]
    ring, final = "u8", C.final(links)
    compat, blur = params(0)
    ref = reference_of(gpu_renderer_factory, "rim-" + kind, dims, links, ring, compat, blur)
    wdata, wgrad = ref.steps[final]
    nz, ny, nx = dims[::-1]
    stale, sgrad = np.full((nz, ny, nx, 3), 255, np.uint8), np.full((nz, ny, nx, 3), 7, np.uint8)
    sc = T.scene(wdata, wgrad)
    opts = (("kernel", 1),)
    dm = dmode_of(links)
    ranks = [C.Rank(dims, r, nranks, halo, ring) for r in range(nranks)]
    want = []
    for K in ranks:
        st = C.run(K, links)[final]
        assert (K.stored() & ~st.mask).any() and C.telling_faces(K, st), "a rim at a telling face"
        both = []
        for fill, gfill in ((0, 128), (255, 7)):            # the result with its rim zeroed; with the stale step left on it
            d, g = wdata.copy(), wgrad.copy()
            d[~st.mask], g[~st.mask] = fill, gfill
            U = rank_context(gpu_renderer_factory, dims, d, g, dmode(kind, d.shape[-1]), K.rank, nranks, halo, opts=opts)
            try:
                both.append(flags_of(U, sc, 0, rim_tables()))
            finally:
                U.close()
        want.append(both)
    rs = declared_ranks(gpu_renderer_factory, ranks, dm, opts=opts)
    try:
        before = []
        for R in rs:
            R.upload_timestep(final, stale, sgrad, fsize=fsz(dims), dmode=dm)
            before.append(flags_of(R, sc, final, rim_tables()))
        words, keep = run_chain(smk, rs, ranks, links, ring, compat, blur)
        got = [flags_of(R, sc, final, rim_tables()) for R in rs]
        assert all(R.timesteps()[0] == final for R in rs)      # (the shown step, overwritten in place)
        del words, keep
    finally:
        close(rs)
    seen = [False, False]
    for K, b, g, (zeroed, left) in zip(ranks, before, got, want):
        assert b[0].all() and b[1].all(), "the stale step flags every brick under both tables"
        for t in (0, 1):
            assert np.array_equal(g[t], zeroed[t]), "rank %d, table %d: %d bricks differ from the zeroed rim's" % (K.rank, t, (g[t] != zeroed[t]).sum())
            seen[t] |= not np.array_equal(left[t], zeroed[t])
        assert not np.array_equal(left[1], zeroed[1]), "rank %d: the second table tells a stale rim from a zeroed one" % K.rank
    assert all(seen), "both tables tell a stale rim from a zeroed one on some rank: %s" % seen


# ---- 3. the witness of sensitivity

TWO_RANKS = [pytest.param(i, ring, id="%s-%s" % (C.CASE_IDS[i], ring)) for i in range(len(C.CASES)) for ring in C.RINGS
             if C.CASES[i][2] == 2 and C.CASE_IDS[i] not in C.NO_TELLING_FACE]


@pytest.mark.parametrize("case, ring", TWO_RANKS)
def test_a_rim_fed_voxel_differs_from_the_exact_one(gpu_renderer_factory, case, ring):
    import torch
    cid, dims, nranks, halo, links = C.CASES[case]
    compat, blur = params(case)
    ref = reference(gpu_renderer_factory, case, ring)
    dm = dmode_of(links)
    told = 0
    for K in C.ranks_of(case, ring):
        for out, st in C.run(K, links).items():
            faces = C.telling_faces(K, st)
            if not faces:
                continue
            kind, src_id = st.link[2], st.link[3]
            data, grad = ref.steps[src_id]
            zd, zg = data.copy(), grad.copy()
            zd[~st.src], zg[~st.src] = 0, 128               # what the rank holds of the source: zeros on its rim
            assert zd[st.src].any() and data[~st.src].any()
            W = declared(gpu_renderer_factory, dims, ring, 3, dm, cap=4)
            try:
                W.upload_timestep(1, data, grad, fsize=fsz(dims), dmode=dm)
                W.upload_timestep(2, zd, zg, fsize=fsz(dims), dmode=dm)
                same(W.download_timestep(1)[0], data, "the source, read back and uploaded again")
                w = words_buf()
                W.step_extremes_device(0 if kind == "derive" else 1, 1, w.data_ptr(), compat=compat)
                torch.cuda.synchronize()                    # the export ran on the context's stream: read-back
                assert np.array_equal(w.cpu().numpy()[0], ref.words[out])
                write_shard(W, kind, 2, 3, w.data_ptr(), compat, blur)
                got = W.download_timestep(3)
            finally:
                W.close()
            wdata, wgrad = ref.steps[out]
            differ = (D.bits(got[0]) != D.bits(wdata)).any(-1) | (got[1] != wgrad).any(-1)
            assert not (differ & st.mask).any(), "%s rank %d step %d: %d voxels of the model's box depend on the source's rim" % (
                cid, K.rank, out, (differ & st.mask).sum())
            for face in faces:
                layers = C.between(K, st, face)
                n = int((differ & layers).sum())
                print("WITNESS %s %s rank %d step %d face %s%s: %d of %d voxels between the source's box and the model's differ" % (
                    cid, ring, K.rank, out, "xyz"[face[0]], "-+"[face[1]], n, layers.sum()))
                assert n > 0, "%s rank %d step %d face %s: the data cannot tell a rim-fed voxel from an exact one" % (cid, K.rank, out, face)
                told += 1
    assert told


# ---- 4. frames of the final step

FRAMES = [("B-derive-12x9x13-r2-h6", "u8"), ("C-derive-12x9x13-r2-h6", "f32"), ("D-21x9x13-r2-h4", "u16")]


@pytest.mark.parametrize("bricks", [0, 1])
@pytest.mark.parametrize("kernel", [1, 2], ids=["gather", "slice-ring"])
@pytest.mark.parametrize("cid, ring", FRAMES)
def test_frames_of_the_chains_final_step(gpu_renderer_factory, smk, cid, ring, kernel, bricks):
    from _scenes import push_scene
    case = C.CASE_IDS.index(cid)
    _, dims, nranks, halo, links = C.CASES[case]
    compat, blur = params(case)
    ref = reference(gpu_renderer_factory, case, ring)
    final, kind = C.final(links), C.final_kind(links)
    wdata, wgrad = ref.steps[final]
    opts = (("kernel", kernel), ("bricks", bricks), ("slab_split", 1))
    sc = T.scene(wdata, wgrad)

    def frames(rs):
        for R in rs:
            push_scene(R, sc, upload=False)
        lay, out = merged(rs, sc)
        assert all(R.last_frame_info()[0] == RAN[kernel] for R in rs) and all(R.stat("slab_failures") == 0 for R in rs)
        return lay, out
    up = ranks_of(gpu_renderer_factory, dims, wdata, wgrad, dmode(kind, wdata.shape[-1]), nranks, halo, opts=opts)     # ... that UPLOADED the unsharded result
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
    ranks = C.ranks_of(case, ring)
    rs = declared_ranks(gpu_renderer_factory, ranks, dmode_of(links), opts=opts)
    try:
        frames(rs)                                          # (the declared zeros rendered first: flags and plans of another step exist)
        words, keep = run_chain(smk, rs, ranks, links, ring, compat, blur)
        for R in rs:
            R.select_timestep(final)
        got_layers, got = frames(rs)
        del words, keep
    finally:
        close(rs)
    assert whole[..., 3].max() > 0.05 and all(l[..., 3].max() > 0.01 for l in want_layers)
    for r in range(nranks):                                 # (a rim is never sampled: the layers are those of the uploaded result)
        assert np.array_equal(got_layers[r], want_layers[r]), "rank %d: max diff %g" % (r, np.abs(got_layers[r] - want_layers[r]).max())
    assert np.array_equal(got, want)
    err = np.abs(got - whole).max()
    assert err <= G.SORT_LAST_TOL, "merged against the unsharded frame: max abs err %g" % err


# ---- 5. chains whose halo runs out

@pytest.mark.parametrize("n", range(len(C.REFUSED)), ids=C.REFUSED_IDS)
def test_a_chain_whose_halo_runs_out_is_refused(gpu_renderer_factory, smk, n):
    from _scenes import push_scene
    cid, dims, nranks, halo, links, refused, (have, reach) = C.REFUSED[n]
    ring = "u8"
    _, out, kind, src_id = refused
    dm = dmode(kind, 3)
    src, fields = sources(ring, dims)
    sc = T.scene(*src[0])
    ranks = [C.Rank(dims, r, nranks, halo, ring) for r in range(nranks)]
    for K in ranks:
        with pytest.raises(C.Refused):
            C.run(K, links + (refused,))
    w = words_buf()
    p = w.data_ptr()
    why = r"smk_%s: time step %d \(the source\) has a valid halo of %d voxels, the stencil reaches %d .*a valid halo >= %d is needed"
    rs = declared_ranks(gpu_renderer_factory, ranks, dm, opts=(("kernel", 1),))
    try:
        keep = []
        for link in links:
            sharded_link(smk, rs, ranks, link, src, fields, dm, 1, 0, keep)
        for R, K in zip(rs, ranks):
            assert R.timestep_halo(src_id) == have == C.run(K, links)[src_id].halo
            push_scene(R, sc, upload=False)
            with Undisturbed(R):
                with pytest.raises(smk.SmkError, match=why % ("step_extremes_device", src_id, have, reach, reach + 1)):
                    R.step_extremes_device(0 if kind == "derive" else 1, src_id, p)
                with pytest.raises(smk.SmkError, match=why % (kind + "_timestep_shard", src_id, have, reach, reach + 1)):
                    write_shard(R, kind, src_id, out, p)
        del keep
    finally:
        close(rs)
    assert (w.cpu().numpy() == 0x5a5a5a5a).all(), "a refused export writes no word"
