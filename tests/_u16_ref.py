"""SMK_U16 voxels (include/smk.h): the layout, its decode and the float -> u16 rule restated in numpy, volumes that use all
sixteen bits, and the cases shared by tests/test_u16_cpu.py (which qualifies them on the CPU checker alone) and
tests/test_gpu_u16.py (which renders them).  TEST INFRASTRUCTURE ONLY.

The packed voxel is 8 bytes,
    uint2 { c0 | c1 << 16,   n0 | n1 << 8 | n2 << 16 | q8(c2) << 24 },   q8(c) = (c * 255 + 32767) // 65535,
and a sample's channels are c0 / 65535, c1 / 65535, q8(c2) / 255.  The CPU checker has no such type: it renders
decode_u16(volume) as an f32 volume.  The product interpolates the raw integers and scales once, the checker scales every
voxel and interpolates; both are a handful of fp32 roundings of values <= 1, i.e. they differ by at most a few 2^-24
(measured on 4e6 random cells: 2.4e-7) in a channel value."""
import functools

import numpy as np

import oracle as O
import _layouts as L

DIMS_EVEN, DIMS_ODD, DIMS_33 = (32, 24, 26), (23, 27, 29), (33, 25, 24)
TOL = 1e-4


# ------------------------------------------------------------------------------------------------ the layout

def q8(c):
    """the nearest 8-bit unorm of a 16-bit one, in integer arithmetic"""
    return ((np.asarray(c).astype(np.uint32) * 255 + 32767) // 65535).astype(np.uint8)


def pack_u16(data, grad=None):
    """[z][y][x][nelts] uint16 (+ [z][y][x][3] u8 normals) -> the packed voxels, [z][y][x][2] uint32"""
    data = np.asarray(data)
    assert data.dtype == np.uint16 and 1 <= data.shape[-1] <= 3
    ne = data.shape[-1]
    out = np.zeros(data.shape[:-1] + (2,), np.uint32)
    out[..., 0] = data[..., 0]
    if ne > 1:
        out[..., 0] |= data[..., 1].astype(np.uint32) << 16
    if grad is None:
        out[..., 1] = 0x808080
    else:
        g = np.asarray(grad).astype(np.uint32)
        out[..., 1] = g[..., 0] | (g[..., 1] << 8) | (g[..., 2] << 16)
    if ne > 2:
        out[..., 1] |= q8(data[..., 2]).astype(np.uint32) << 24
    return out


def decode_u16(data):
    """the channel values of u16 voxels as float32 [..., nelts]"""
    data = np.asarray(data)
    assert data.dtype == np.uint16
    out = np.zeros(data.shape, np.float32)
    for e in range(data.shape[-1]):
        if e < 2:
            out[..., e] = data[..., e].astype(np.float32) / np.float32(65535.0)
        else:
            out[..., e] = q8(data[..., e]).astype(np.float32) / np.float32(255.0)
    return out


def quantize_u16(v):
    """smk_quantize_u16_device's rule in float32: t = v * 65535; NaN or t < 0 -> 0, t >= 65535 -> 65535, else
    (uint16)(int)(t + 0.5)"""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v * np.float32(65535.0)).astype(np.float32)
        mid = (t >= 0) & (t < np.float32(65535.0))
        r = (np.where(mid, t, np.float32(0)) + np.float32(0.5)).astype(np.float32)
        out = np.where(mid, r.astype(np.int32), 0)
    out = np.where(t >= np.float32(65535.0), 65535, out)       # (NaN compares false everywhere: 0)
    return out.astype(np.uint16)


def quantize_file16(native):
    """VolumeFiles' quantize_to_u16 restated: the file's own min/max onto 0..65535 in double, truncated; a constant volume 0"""
    x = np.asarray(native).astype(np.float64)
    lo, hi = x.min(), x.max()
    if hi == lo:
        return np.zeros(x.shape, np.uint16)
    return (65535.0 * (x - lo) / (hi - lo) + 0.0).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ volumes

@functools.lru_cache(maxsize=None)
def volume16(dims=DIMS_EVEN, seed=3):
    """([z][y][x][3] uint16, normals [z][y][x][3] u8): a value field over the whole 16-bit range with noise far below one
    8-bit step (257 raw units) on top, its gradient magnitude, and a third field that does not depend on them"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.sin(x * .31 + .2 * seed) + np.cos(y * .23) + np.sin(z * .41 + x * .07)
    v = (v - v.min()) / (v.max() - v.min())
    c0 = np.clip(np.round(v * 65535.0) + rng.integers(-90, 91, v.shape), 0, 65535)
    c0.flat[np.argmin(v)] = 0
    c0.flat[np.argmax(v)] = 65535
    gz, gy, gx = np.gradient(v)
    g = np.sqrt(gx * gx + gy * gy + gz * gz)
    c1 = np.round(g / g.max() * 65535.0)
    c2 = np.round((.5 + .5 * np.sin(.5 * x + .3 * y + 1.3 * (seed - 3) + .2 * z)) * 65535.0)
    d = np.ascontiguousarray(np.stack([c0, c1, c2], -1).astype(np.uint16))
    assert d[..., 0].min() == 0 and d[..., 0].max() == 65535 and len(np.unique(d[..., 0] & 0xff)) > 200
    nrm = O.normals_vgh(np.ascontiguousarray(q8(d)), blur=True)
    d.setflags(write=False)
    nrm.setflags(write=False)
    return d, nrm


@functools.lru_cache(maxsize=None)
def table_1d():
    """a 256-entry 1-D colour table (straight RGBA, as TLUT::_rgba holds it) whose premultiplied neighbours differ by less
    than 4e-5 in every component.  The lookup is nearest-neighbour, index (int)(ch0 * 255 + .5): where the two arithmetic
    orders of the channel value (see the module's head) fall on different sides of a half-integer -- measured 6e-6 of the
    samples -- the product and the checker read neighbouring entries, and that may not cost the 1e-4 tolerance.  A wrong
    decode moves the index by tens of entries at every sample, which it does cost"""
    i = np.arange(256) / 255.0
    t = np.stack([.2 + .2 * i, .5 + 0 * i, .9 - .2 * i, .03 + .006 * i], -1).astype(np.float32)
    pm = t[:, :3] * t[:, 3:]
    assert np.abs(np.diff(pm, axis=0)).max() < 4e-5 and np.abs(np.diff(t[:, 3])).max() < 4e-5
    t.setflags(write=False)
    return t


class Case:
    """a u16 volume, and the checker's scene of its decoded values (sc.data float32); sc.dmode as in _layouts.scene"""

    def __init__(self, vol16, sc):
        self.vol16, self.sc = vol16, sc


def case(nelts, table="2d", shade=0, view="rot", window=(48, 48), dims=DIMS_EVEN, seed=3, grad=True, mode=None):
    """table: '1d' (table_1d), or _layouts.tables' '2d' / '2d3' / '3d'; 48 planes"""
    d, nrm = volume16(tuple(dims), seed)
    vol16 = np.ascontiguousarray(d[..., :nelts])
    sc = O.Scene(decode_u16(vol16), grad=nrm if grad else None)
    if table == "1d":
        sc.tf_mode, sc.tlut = 0, table_1d()
    else:
        sc.tf_mode, sc.tf_vg, sc.tf_h, sc.tf3d = L.tables(table)
    sc.dmode = mode or L.DEFAULT_MODE[nelts]
    sc.third_axis = L.third_axis(sc.dmode, nelts, sc.tf_h)
    sc.width, sc.height = window
    sc.steps = 48
    sc.shade_mode = shade
    L.pose(sc, view)
    return Case(vol16, sc)


# (nelts, table, shade, view, blend, depth, dims): every channel count, table kind, shading and blend, first-hit depth
# (under tables whose alpha is nowhere 0, so that the first sample is the first one inside the volume for both
# arithmetic orders), both principal-axis families (views along x take the x-major copy on the slice-ring kernel)
PARITY = (
    (1, "1d", 0, "rot", 0, False, DIMS_EVEN),
    (1, "1d", 0, "x+", 1, False, DIMS_ODD),
    (1, "2d", 0, "z-", 0, True, DIMS_ODD),
    (2, "2d", 1, "x+", 0, False, DIMS_EVEN),
    (2, "2d", 2, "y-", 1, True, DIMS_33),
    (2, "2d", 0, "rot", 2, False, DIMS_ODD),
    (3, "2d3", 1, "rot", 0, True, DIMS_EVEN),
    (3, "2d3", 2, "x-", 2, False, DIMS_ODD),
    (3, "2d3", 0, "close", 1, False, DIMS_33),
    (3, "3d", 1, "y+", 0, False, DIMS_ODD),
    (3, "3d", 2, "x+", 1, False, DIMS_EVEN),
    (3, "3d", 0, "diag", 2, False, DIMS_33),
)


def parity_id(c):
    return "n%d-%s-sh%d-%s-b%d%s-%dx%dx%d" % (c[0], c[1], c[2], c[3], c[4], "-depth" if c[5] else "", *c[6])


def parity_case(c):
    nelts, table, shade, view, _, _, dims = c
    return case(nelts, table, shade, view, (64, 48) if view == "close" else (48, 48), dims)


# ------------------------------------------------------------------------------------------------ fine structure

FINE_DIMS = (32, 24, 26)


@functools.lru_cache(maxsize=None)
def fine_volume():
    """two channels: a smooth ramp along x across about eight 8-bit steps around mid-range, plus detail in y and z whose
    amplitude, 0.35 / 255, is below one 8-bit step; the second channel is constant"""
    nx, ny, nz = FINE_DIMS
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = 124.0 / 255 + (x / (nx - 1.0)) * (8.0 / 255) + (.35 / 255) * np.sin(1.1 * y + .4) * np.cos(.9 * z)
    d = np.zeros((nz, ny, nx, 2), np.uint16)
    d[..., 0] = np.round(v * 65535.0)
    d[..., 1] = 32768
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def fine_table():
    """a 256 x 256 2-D table, constant along g, whose alpha rises from 0 to 1 across two texels of the value axis"""
    t = np.zeros((256, 256, 4), np.uint8)
    t[..., 0], t[..., 1], t[..., 2] = 255, 160, 60
    t[:, 128, 3] = 128
    t[:, 129:, 3] = 255
    t.setflags(write=False)
    return t


def fine_case(eight_bit=False):
    """the fine-structure scene; eight_bit: the checker's scene of the same data quantised to 8 bits (a u8 volume)"""
    d = fine_volume()
    sc = O.Scene(np.ascontiguousarray(q8(d)) if eight_bit else decode_u16(d))
    sc.tf_mode, sc.tf_vg = 1, fine_table()
    sc.dmode, sc.third_axis = "V1G", 0
    sc.width = sc.height = 48
    sc.steps = 48
    sc.shade_mode = 0
    L.pose(sc, "rot")
    return Case(d, sc)


# ------------------------------------------------------------------------------------------------ the product's side

def upload(r, c, grid=(1, 1, 1), order=None, to_device=None, timestep=None, stream=None, ready=None):
    """smk_upload_volume[_device] / smk_upload_timestep[_device] of the case's u16 voxels (dtype 2), called directly"""
    sc = c.sc
    descs, keep = descriptors(c.vol16, sc.grad, sc.fsize, grid, order, to_device)
    if ready is not None:
        ready()
    mode = L.MODES.index(sc.dmode)
    if timestep is None:
        f = r.L.smk_upload_volume_device if to_device else r.L.smk_upload_volume
        rc = f(r.ctx, descs, len(descs), sc.nelts, 2, mode)
    elif to_device:
        rc = r.L.smk_upload_timestep_device(r.ctx, int(timestep), descs, len(descs), sc.nelts, 2, mode, stream)
    else:
        rc = r.L.smk_upload_timestep(r.ctx, int(timestep), descs, len(descs), sc.nelts, 2, mode)
    r._ck(rc)
    return keep


# uneven brick boundaries of the all-odd 23 x 27 x 29 volume, by grid (as _layouts.CUTS for its own odd volume); chosen so
# that every last brick's float32 size closes the volume's extent exactly (_layouts._f32_sum_to; test_u16_cpu.py)
CUTS = {(2, 2, 2): ([0, 13, 23], [0, 11, 27], [0, 11, 29]),
        (3, 1, 2): ([0, 6, 15, 23], [0, 27], [0, 17, 29])}


def bricks(dims, fsize, grid):
    """[(ipos, isize, fpos, fsize)] of the tiling CUTS[grid], x fastest (as _layouts.bricks); one brick for (1, 1, 1)"""
    if tuple(grid) == (1, 1, 1):
        axes = tuple([0, n] for n in dims)
    else:
        assert tuple(dims) == DIMS_ODD
        axes = CUTS[tuple(grid)]
    out = []
    for k in range(len(axes[2]) - 1):
        for j in range(len(axes[1]) - 1):
            for i in range(len(axes[0]) - 1):
                idx = (i, j, k)
                ipos = tuple(axes[a][idx[a]] for a in range(3))
                isize = tuple(axes[a][idx[a] + 1] - axes[a][idx[a]] for a in range(3))
                fpos, fs = [], []
                for a in range(3):
                    p = np.float32(np.float32(fsize[a]) * ipos[a] / dims[a])
                    if ipos[a] + isize[a] == dims[a]:
                        s = L._f32_sum_to(fsize[a], p)       # (the extent the single brick states, exactly)
                    else:
                        s = np.float32(np.float32(fsize[a]) * isize[a] / dims[a])
                    fpos.append(float(p))
                    fs.append(float(s))
                out.append((ipos, isize, tuple(fpos), tuple(fs)))
    return out


def descriptors(data, grad, fsize, grid=(1, 1, 1), order=None, to_device=None):
    """(descriptor array, keep-alive list) of the volume cut into bricks(...), handed over in `order`"""
    from simian_spacemonkey_amd.binding import VolumeDesc
    nz, ny, nx, _ = data.shape
    bs = bricks((nx, ny, nz), fsize, grid)
    order = list(range(len(bs))) if order is None else list(order)
    assert sorted(order) == list(range(len(bs)))
    descs = (VolumeDesc * len(bs))()
    keep = []

    def ptr(a):
        a = np.ascontiguousarray(a)
        if to_device is None:
            keep.append(a)
            return a.ctypes.data
        p, owner = to_device(a)
        keep.append(owner)
        return p
    for d, k in zip(descs, order):
        (x0, y0, z0), (bx, by, bz), fpos, fs = bs[k]
        d.xiSize, d.yiSize, d.ziSize = bx, by, bz
        d.xfSize, d.yfSize, d.zfSize = fs
        d.xiPos, d.yiPos, d.ziPos = x0, y0, z0
        d.xfPos, d.yfPos, d.zfPos = fpos
        d.data = ptr(data[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
        d.grad = ptr(grad[z0:z0 + bz, y0:y0 + by, x0:x0 + bx]) if grad is not None else None
    return descs, keep


def frame_state(r, sc):
    """everything of a frame but the volume (as _layouts.frame_state, and the 1-D table)"""
    r.set_option("tf_raw", 1)
    if sc.tf_mode == 0:
        r.set_tlut1d(sc.tlut)
    elif sc.tf_mode == 1:
        r.set_tf2d(sc.tf_vg, sc.tf_h)
    else:
        r.set_tf3d(sc.tf3d)
    r.set_clip(0, None)
    r.set_clip_plane(None)
    r.set_camera(sc.mv(), sc.frustum, (sc.znear, 20.0), sc.width, sc.height)
    r.set_sampling(sc.sample_rate, sc.steps, 1.0, 1)
    m = {0: "none", 1: "r8k" if sc.use_spec else "r8k_diff", 2: "nv20" if sc.use_spec else "nv20_diff"}[sc.shade_mode]
    r.set_shading(m, sc.light_pos, sc.eye, sc.at, sc.xform, sc.intens)
    r.set_perturb(None, None, None)
    if getattr(sc, "shadow", None):
        r.set_shadow(1, *sc.shadow)
    else:
        r.set_shadow(0)


def push(r, c, grid=(1, 1, 1), order=None):
    upload(r, c, grid, order)
    frame_state(r, c.sc)
