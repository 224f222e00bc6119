"""Contexts, comparisons and shared procedures of the GPU tests of the time-step ring (tests/test_gpu_step_*.py,
test_gpu_tblend.py, test_gpu_timesteps.py).  Test modules import from here and from tests/_gpu_mem.py (device buffers: read
its rule first), never from one another.  torch and the product package are imported inside the functions."""
import numpy as np

import _step_block_ref as B
import _step_derive_ref as V
import _step_merge_ref as M
import _step_read_ref as D
import _step_shard_ref as S
import _tblend_ref as T
from _gpu_mem import dev_ptr, merged, out_buffer, words_buf

CODE = M.CODE                                               # smk_dtype of a ring type (every _step_*_ref module has this table)
RAN = {1: 1, 2: 2, 3: 4}                                    # option "kernel" -> what smk_last_frame_info reports
MODE = {2: "V1G", 3: "V2G", 4: "V3G"}                       # the data mode mergeMV -addG gives nelts channels
# A merged sharded frame against the unsharded frame.  The sharded time-step test, tests/test_gpu_timesteps.py::
# test_shards_switch_and_merge, compares merged shards with merged FRESH shards, exactly, and has no tolerance against the
# unsharded frame to take; that exact comparison is made in the step tests too.  Against the unsharded frame this is the
# sort-last tolerance of tests/test_gpu_shadow_shards.py (TOL), the tightest one the suite uses for that comparison
SORT_LAST_TOL = 2e-5


# ---- comparisons

def same_bits(got, want, what=""):
    got, want = D.bits(got), D.bits(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d values differ, first at %s: got %#x, want %#x" % (
        what, len(bad), got.size, tuple(bad[0]), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def same_bins(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d bins differ, first %s: got %d, want %d; totals %d / %d" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])], int(got.astype(np.int64).sum()), int(want.astype(np.int64).sum()))


# ---- small things

def fsz(dims):
    m = float(max(dims))
    return tuple(float(np.float32(n / m)) for n in dims)


def close(rs):
    for R in rs:
        R.close()


def dmode(kind, nelts):
    return "VGH" if kind == "derive" else MODE[nelts]


def _mode(dm, nelts):
    """a data mode, or a table of them by channel count"""
    return dm if isinstance(dm, str) else dm[nelts]


# ---- contexts of a series in its natural extents

def context(factory, data, grad, cap=1, shard=None, halo=None, dm=D.DMODE):
    """a context whose step 0 (current) is (data, grad) in data mode `dm` (or dm[nelts]); grad None: no normals"""
    R = factory()
    try:
        if shard:
            R.set_shard(*shard)
        if halo is not None:
            R.set_option("halo", halo)
        if cap > 1:
            R.set_timestep_cache(cap)
        R.upload_volume(data, grad, dmode=_mode(dm, data.shape[-1]))
    except Exception:
        R.close()
        raise
    return R


def series(factory, steps, cap=4, dm="VGH"):
    """a context whose step 0 (current), 1, ... are `steps` = ((data, grad), ...); grad None: no normals"""
    R = context(factory, steps[0][0], steps[0][1], cap=cap, dm=dm)
    try:
        for t, (data, grad) in enumerate(steps[1:], 1):
            R.upload_timestep(t, data, grad, dmode=_mode(dm, data.shape[-1]))
    except Exception:
        R.close()
        raise
    return R


def ring(factory, a, b, cap=4):
    """a context with step 0 = a (current) and step 1 = b resident in the data mode of their channel count, and the two steps"""
    return series(factory, (a, b), cap, D.DMODE), a, b


def bricked(smk, data, grad, order):
    """(smk_volume_desc array, keep-alive list) of the volume cut at its midpoints into 2 x 2 x 2 unequal bricks, handed over
    in `order`"""
    nz, ny, nx, _ = data.shape
    dims, m = (nx, ny, nz), float(max(nx, ny, nz))
    cuts = [(0, n // 2, n) for n in dims]
    boxes = [[(cuts[a][i[a]], cuts[a][i[a] + 1]) for a in range(3)] for i in np.ndindex(2, 2, 2)]
    descs, keep = (smk.binding.VolumeDesc * 8)(), []
    for d, k in zip(descs, order):
        (x0, x1), (y0, y1), (z0, z1) = boxes[k]
        d.xiSize, d.yiSize, d.ziSize = x1 - x0, y1 - y0, z1 - z0
        d.xfSize, d.yfSize, d.zfSize = (x1 - x0) / m, (y1 - y0) / m, (z1 - z0) / m
        d.xiPos, d.yiPos, d.ziPos = x0, y0, z0
        d.xfPos, d.yfPos, d.zfPos = x0 / m, y0 / m, z0 / m
        sub = [np.ascontiguousarray(a[z0:z1, y0:y1, x0:x1]) for a in (data, grad)]
        keep += sub
        d.data, d.grad = sub[0].ctypes.data, sub[1].ctypes.data
    return descs, keep


def scene_context(factory, sc, cap=None, shard=None):
    """a context that can render: scene sc pushed (its volume is step 0, current)"""
    from _scenes import push_scene
    R = factory()
    try:
        if shard:
            R.set_shard(*shard)
        if cap:
            R.set_timestep_cache(cap)
        push_scene(R, sc)
    except Exception:
        R.close()
        raise
    return R


def fresh_frame(factory, sc, opts=(), render=None):
    from _scenes import push_scene
    R = factory()
    try:
        push_scene(R, sc)
        for k, v in opts:
            R.set_option(k, v)
        if render:
            return render(R)
        out = R.render()
        assert R.stat("slab_failures") == 0
        return out
    finally:
        R.close()


def merged_frame(rs, sc, shadow):
    """the ranks' frame: with shadows the light exchange's, else the composite of their layers"""
    from simian_spacemonkey_amd import sortlast
    if shadow:
        return sortlast.render_shadow_frame_local(rs).cpu().numpy()
    return merged(rs, sc)[1]


def fresh_download(factory, data, nrm, dm, normals=True):
    """the download of a fresh context that uploaded (data, nrm) from device memory"""
    nz, ny, nx, ne = data.shape
    F = factory()
    try:
        pd, k0 = dev_ptr(data)
        pn, k1 = dev_ptr(nrm)
        F.upload_volume_device(pd, (nx, ny, nz), ne, CODE[M.RING_OF[data.dtype]], pn if normals else None, dmode=_mode(dm, ne))
        return F.download_timestep()
    finally:
        F.close()


def recipe(R, s, ring, compat, blur):
    """what the device entries of the recipe "Derivatives of a blend" make of the scalar s [z][y][x] (u8, u16 or f32) for a ring
    of type `ring`: (data, normals) as host arrays, made on the device through context R"""
    nz, ny, nx = s.shape
    dims, n = (nx, ny, nz), nx * ny * nz
    ps, keep = dev_ptr(s)
    v8 = out_buffer(n * 3, np.uint8)                        # (the entries run on the context's stream)
    vf = out_buffer(n * 3, np.float32)
    nrm = out_buffer(n * 3, np.uint8)
    q = out_buffer(n * 3 * 2, np.uint8)
    R.make_vgh_device(ps, V.CODE[{np.uint8: "u8", np.uint16: "u16", np.float32: "f32"}[s.dtype.type]], dims, compat, v8.data_ptr(), vf.data_ptr())
    if ring == "u8":
        R.normals_vgh_device(v8.data_ptr(), 3, dims, blur, nrm.data_ptr())
        data = v8.cpu().numpy()
    else:
        R.normals_f32_device(vf.data_ptr(), 3, dims, blur, nrm.data_ptr())
        if ring == "u16":
            R.quantize_u16_device(vf.data_ptr(), n * 3, q.data_ptr())
            data = q.cpu().numpy().view(np.uint16)
        else:
            data = vf.cpu().numpy()
    return data.reshape(nz, ny, nx, 3), nrm.cpu().numpy().reshape(nz, ny, nx, 3)


def recipe_download(factory, R, s, ring, compat, blur, normals=True):
    return fresh_download(factory, *recipe(R, s, ring, compat, blur), "VGH", normals=normals)


# ---- contexts with the series' extents given: one rank of `nranks`, or unsharded

def _rank(factory, rank, nranks, halo, cap, opts, first):
    R = factory()
    try:
        if nranks > 1:
            R.set_shard(rank, nranks)
            R.set_option("halo", halo)
        for k, v in opts:
            R.set_option(k, v)
        R.set_timestep_cache(cap)
        first(R)
    except Exception:
        R.close()
        raise
    return R


def rank_context(factory, dims, data, grad, dm, rank=0, nranks=1, halo=1, cap=4, opts=()):
    """a context (one rank of `nranks`, or unsharded) whose step 0 is the UPLOADED (data, grad); grad None: no normals"""
    return _rank(factory, rank, nranks, halo, cap, opts, lambda R: R.upload_volume(data, grad, fsize=fsz(dims), dmode=dm))


def declared(factory, dims, ring, nelts, dm, rank=0, nranks=1, halo=1, normals=True, cap=4, opts=()):
    """... that was given the series' geometry and no data"""
    return _rank(factory, rank, nranks, halo, cap, opts,
                 lambda R: R.declare_volume(dims, nelts, CODE[ring], fsize=fsz(dims), dmode=dm, normals=normals))


def uploaded_zeros(factory, dims, ring, nelts, dm, rank=0, nranks=1, halo=1, normals=True, cap=4, opts=()):
    """... that UPLOADED a volume of zeros: existing entries alone"""
    nx, ny, nz = dims
    return _rank(factory, rank, nranks, halo, cap, opts, lambda R: R.upload_volume(
        np.zeros((nz, ny, nx, nelts), M.NP[ring]), np.full((nz, ny, nx, 3), 128, np.uint8) if normals else None, fsize=fsz(dims), dmode=dm))


def _ranks(make, n):
    rs = []
    try:
        for r in range(n):
            rs.append(make(r))
    except Exception:
        close(rs)
        raise
    return rs


def ranks_of(factory, dims, data, grad, dm, nranks, halo, cap=4, opts=()):
    return _ranks(lambda r: rank_context(factory, dims, data, grad, dm, r, nranks, halo, cap, opts), nranks)


def ranks_declared(factory, dims, ring, nelts, dm, cuts, normals=True, cap=4, opts=()):
    """the declared rank of every element of `cuts`: the cuts of tests/_step_block_ref.py, or the ranks of tests/_step_chain_ref.py
    (anything with .rank, .nranks and .option_halo)"""
    return _ranks(lambda i: declared(factory, dims, ring, nelts, dm, cuts[i].rank, cuts[i].nranks, cuts[i].option_halo, normals, cap, opts),
                  len(cuts))


def pert_scene(data, grad):
    sc = T.scene(data, grad, pert=True)
    sc.pert_w = (.04, .02, 0, 0)
    return sc


def pert_need(dims, w):
    return [1 + int(np.ceil(0.5 * (abs(w[0]) + abs(w[1])) * n)) for n in dims]


# ---- refusals change nothing

class Undisturbed:
    """the refusals inside the block change nothing: the context renders, flags its bricks, lists and downloads its steps as before"""

    def __init__(self, R, visible=True):
        self.R, self.visible = R, visible

    def state(self):
        R = self.R
        frame = R.render()
        return frame, R.brick_flags()[0], R.timesteps(), [R.download_timestep(t) for t in R.timesteps()[1]], R.stat("tblend_count")

    def __enter__(self):
        self.before = self.state()
        assert not self.visible or self.before[0][..., 3].max() > 0.05
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        after = self.state()
        assert np.array_equal(after[0], self.before[0]), "the frame after the refusals"
        assert np.array_equal(after[1], self.before[1]), "the brick flags after the refusals"
        assert after[2] == self.before[2] and after[4] == self.before[4]
        for (d0, g0), (d1, g1) in zip(self.before[3], after[3]):
            same_bits(d1, d0, "a step after the refusals")
            same_bits(g1, g0, "its normals after the refusals")
        return False


class UndisturbedHalos:
    """the same for the shard and block entries: the context renders, lists its steps and reports their valid halos as before,
    and (downloads) downloads them as before.  Not one class with Undisturbed: that one also holds the brick flags and the blend
    count, which these tests never held, and wants a visible frame"""

    def __init__(self, R, downloads=True):
        self.R, self.downloads = R, downloads

    def state(self):
        R = self.R
        ids = R.timesteps()
        return R.render(), ids, [R.download_timestep(t) for t in ids[1]] if self.downloads else [], [R.timestep_halo(t) for t in ids[1]]

    def __enter__(self):
        self.before = self.state()
        return self

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        after = self.state()
        assert np.array_equal(after[0], self.before[0]) and after[1] == self.before[1] and after[3] == self.before[3]
        for (d0, g0), (d1, g1) in zip(self.before[2], after[2]):
            same_bits(d1, d0, "a step after the refusals")
            same_bits(g1, g0, "its normals after the refusals")
        return False


# ---- the stencil producers on ranks: tests/test_gpu_step_shard.py's procedures

def export(R, kind, src, compat=1, stream=None):
    import torch
    w = words_buf()
    R.step_extremes_device(0 if kind == "derive" else 1, src, w.data_ptr(), compat=compat, stream=stream)
    torch.cuda.synchronize()                                # the export ran on the context's stream, or the caller's: read-back
    return w.cpu().numpy()[0]


def one_call(R, kind, src, out, compat=1, blur=0, stream=None):
    if kind == "derive":
        R.derive_timestep(src, out, compat, blur, stream=stream)
    else:
        R.merge_timestep(src, out, stream=stream)


def write_shard(R, kind, src, out, d_words, compat=1, blur=0, stream=None):
    if kind == "derive":
        R.derive_timestep_shard(src, out, d_words, compat, blur, stream=stream)
    else:
        R.merge_timestep_shard(src, out, d_words, stream=stream)


_SOURCE_REF = {}


def reference_of_source(factory, kind, ring, dims, nf=2, compat=1, blur=0, normals=True):
    """what the one-call entry makes of the case's source on an unsharded context, made once and shared:
    (source data, source normals, result data, result normals, the unsharded export's words, probe(cells) of the result)"""
    key = (kind, ring, dims, nf, compat, blur, normals)
    if key not in _SOURCE_REF:
        data, grad = S.source(kind, ring, dims, nf)
        grad = grad if normals else None
        U = rank_context(factory, dims, data, grad, dmode(kind, data.shape[-1]))
        try:
            one_call(U, kind, 0, 1, compat, blur)
            got = U.download_timestep(1)
            words = export(U, kind, 0, compat)
            cells = S.cells_of((0, 0, 0), dims)
            probe = U.probe_step(cells, 1)
            assert probe[2].all()
        finally:
            U.close()
        for a in got + probe[:2]:
            a.setflags(write=False)
        _SOURCE_REF[key] = (data, grad, got[0], got[1], words, probe)
    return _SOURCE_REF[key]


def probe_at(ref_probe, dims, cells):
    """the rows of the unsharded probe of every cell of the volume that belong to `cells`"""
    nx, ny, nz = dims
    idx = (cells[:, 0] * (ny - 1) + cells[:, 1]) * (nz - 1) + cells[:, 2]      # (cells_of's order: x slowest)
    return ref_probe[0][idx], ref_probe[1][idx]


def params(kind, i):
    """(compat, blur) of case i: every derive flag takes both values over the case list"""
    return ((1, 0), (0, 1), (1, 1), (0, 0))[i % 4] if kind == "derive" else (1, 0)


def flags_of(R, sc, step, tables):
    """the brick flags of `step` under each of the 2-D tables (made for every table; a frame uses them when few bricks are flagged)"""
    from _scenes import push_scene
    push_scene(R, sc, upload=False)
    R.select_timestep(step)
    out = []
    for t in tables:
        R.set_tf2d(t, None)
        out.append(R.brick_flags()[0].copy())
    return out


def rim_table(opaque):
    t = np.zeros((256, 256, 4), np.uint8)
    if opaque == "all but zero":
        t[...] = 255
        t[:6, :6, 3] = 0                                    # (the bilinear lookup of value 0 reaches texels 0 and 1, and a brick's range is taken
                                                            # with a margin: the lowest few values are transparent)
    else:
        t[250:, 250:] = 255                                 # "the top alone"
    return t


def rim_tables():
    """the two tables under which a rim shows in the brick flags (tests/test_gpu_step_block.py, 4b)"""
    return [rim_table(opaque) for opaque in ("all but zero", "the top alone")]


# ---- ... from a rank's own blocks: tests/test_gpu_step_block.py's procedures

def hand_over(smk, c, whole, ring):
    """(device address of the block's first element, what keeps it alive, the smk_block) of cut c of `whole` [z][y][x](...)"""
    a, off, py, pz = c.take(whole, B.POISON[ring])
    p, keep = dev_ptr(a)
    per = a.itemsize * int(np.prod(a.shape[3:], dtype=np.int64))
    return p + off * per, keep, smk.smk_block(c.origin, c.size, py, pz)


def arrays(kind, ring, dims, sd, nf):
    """the whole dense arrays [z][y][x] a simulation holds: one scalar of type sd (derive), nf fields of the ring's (merge)"""
    if kind == "derive":
        return [B.scalar(sd, dims)]
    F = B.M.fields(ring, nf, dims)
    return [np.ascontiguousarray(F[..., e]) for e in range(nf)]


_ARRAYS_REF = {}


def reference_of_arrays(factory, kind, ring, dims, sd=None, nf=2, compat=1, blur=0, normals=True):
    """what the unsharded one-call entry makes of the whole arrays, made once and shared: (the arrays, result data, result
    normals, probe(cells) of the result, the words an unsharded f32-ring context exports for the same arrays held as floats)"""
    sd = sd or ring
    key = (kind, ring, dims, sd, nf, compat, blur, normals)
    if key not in _ARRAYS_REF:
        arr = arrays(kind, ring, dims, sd, nf)
        nelts = 3 if kind == "derive" else nf + 1
        held = [dev_ptr(a) for a in arr]
        U = uploaded_zeros(factory, dims, ring, nelts, dmode(kind, nelts), normals=normals)
        try:
            if kind == "derive":
                U.upload_timestep_scalar_device(1, held[0][0], CODE[sd], dims, compat, blur)
            else:
                U.upload_timestep_fields_device(1, [h[0] for h in held], CODE[ring], dims)
            got = U.download_timestep(1)
            probe = U.probe_step(S.cells_of((0, 0, 0), dims), 1)
            assert probe[2].all() and got[0].any()
        finally:
            U.close()
        wkey = (kind, dims, sd if kind == "derive" else ring, nf, compat)
        if wkey not in _ARRAYS_REF:                         # the same values as floats in an f32 ring: exact for u8 and u16
            fl = np.stack([a.astype(np.float32) for a in arr] + [np.zeros(dims[::-1], np.float32)] * (nelts - len(arr)), -1)
            W = rank_context(factory, dims, np.ascontiguousarray(fl), None, dmode(kind, nelts))
            try:
                _ARRAYS_REF[wkey] = export(W, kind, 0, compat)
            finally:
                W.close()
        for a in list(got) + list(probe[:2]) + arr:
            a.setflags(write=False)
        _ARRAYS_REF[key] = (arr, got[0], got[1], probe, _ARRAYS_REF[wkey])
    return _ARRAYS_REF[key]


def run_cut(smk, rs, cuts, kind, ring, sd, arr, out, compat, blur, stream=None, **flags):
    """every rank's block (a view: everything outside it is poison) of cut `cuts` handed over: the two passes, then what keeps
    the blocks alive and the words; flags: the add_h of kind merge_h"""
    from simian_spacemonkey_amd import sortlast
    keep, blocks = [], []
    for c in cuts:
        ptrs = []
        for a in arr:
            p, k, blk = hand_over(smk, c, a, sd)
            ptrs.append(p)
            keep.append(k)
        blocks.append((ptrs, CODE[sd], blk))
    words = sortlast.stencil_block_local(rs, kind, blocks, out, compat=compat, blur=blur, stream=stream, **flags)
    return keep, words
