"""The voxel layouts the product accepts and the suite did not render -- nelts 1..4, u8 and f32, with and without
normals, the 13 data modes, bricks of any tiling -- as cases shared by tests/test_layouts_cpu.py (which qualifies them on
the CPU checker alone) and tests/test_gpu_layouts.py (which renders them on the three ray-marchers and the slice quad).
TEST INFRASTRUCTURE ONLY.

The volumes are 20 x 14 x 11 and an all-odd 21 x 13 x 7 (u8 rows are padded to even lengths in x and y): the three
channels of _scenes.ragged_vgh plus a fourth that does not depend on them; a thinner layout is the leading channels of
the same arrays.  The third-axis tables vary along BOTH their axes -- _scenes.tf_h varies with the third channel only,
so a kernel that read the wrong fourth channel could not show."""
import functools

import numpy as np

import oracle as O
from _scenes import POSES, ragged_vgh, tf3d_dense, tf_cfg2

DIMS, DIMS_ODD = (20, 14, 11), (21, 13, 7)
WINDOWS = ((37, 29), (93, 41))          # never a multiple of 16 in both directions

# gluvvDataMode in gluvv.h's order (:221-235), and the modes whose alpha is multiplied by the third-axis table: the cases of
# the reference's switch, NV20VolRen3D.cpp:686-693
MODES = ("V1", "V1G", "V1GH", "V2", "V2G", "V2GH", "V3", "V3G", "V4", "VGH", "VGH_VG", "VGH_V", "UNKNOWN")
THIRD = ("VGH", "V1GH", "V2G", "V2GH", "V3", "V3G", "V4")
DEFAULT_MODE = {1: "V1", 2: "V1G", 3: "VGH", 4: "V2GH"}


# ------------------------------------------------------------------------------------------------ volumes

@functools.lru_cache(maxsize=None)
def _four(dims, seed):
    vgh8, vghf, nrm = ragged_vgh(dims, seed=seed)
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c3 = np.sin(.5 * x + .3 * y + 1.3 * (seed - 3)) * 100 + 128
    u8 = np.ascontiguousarray(np.concatenate([vgh8, np.clip(c3, 0, 255).astype(np.uint8)[..., None]], -1))
    f32 = np.ascontiguousarray(np.concatenate([vghf, np.clip(c3 / 255.0, 0, 1).astype(np.float32)[..., None]], -1))
    assert f32.min() >= 0.0 and f32.max() <= 1.0
    for a in (u8, f32, nrm):
        a.setflags(write=False)
    return u8, f32, nrm


def layout(nelts, f32, dims=DIMS, seed=3):
    """(data [z][y][x][nelts], normals [z][y][x][3]): the leading channels of the four-channel volume"""
    u8, f, nrm = _four(tuple(dims), seed)
    return np.ascontiguousarray((f if f32 else u8)[..., :nelts]), nrm


# ------------------------------------------------------------------------------------------------ tables

@functools.lru_cache(maxsize=None)
def tf_ramp(sv=256, sg=256):
    """the first table: the colours of the reference's default ramp (_scenes.tf_cfg2) under an alpha that varies along v
    and g and is not 0 in the g = 0 row -- a one-channel volume under a 2-D table samples that row alone, where the
    default ramp and _scenes.tf_cfg3 are transparent.  Other sizes are that table resampled (nearest)"""
    t = tf_cfg2()[0].copy()
    v, g = np.arange(256)[None, :], np.arange(256)[:, None]
    t[..., 3] = np.round(255 * (.05 + .3 * g / 255.0 + .3 * (.5 + .5 * np.sin(.07 * v)) ** 2))
    if (sv, sg) != (256, 256):
        t = t[(np.arange(sg) * 256) // sg][:, (np.arange(sv) * 256) // sv]
    t = np.ascontiguousarray(t)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def tf_third(sv=256, sg=256):
    """a third-axis table whose alpha varies along both axes: s is the third channel, t the fourth"""
    s = (np.arange(sv) + .5) / sv
    t = (np.arange(sg) + .5) / sg
    a = (.15 + .85 * (.5 + .5 * np.sin(9.0 * s + 1.0))[None, :] * (.5 + .5 * np.cos(7.0 * t + .4))[:, None])
    tex = np.zeros((sg, sv, 4), np.uint8)
    tex[..., :3] = 255
    tex[..., 3] = np.round(a * 255)
    tex.setflags(write=False)
    return tex


# A pair of tables of another size.  The slice-ring planner keeps the third-axis alpha row in LDS for sv <= 2048
# (smk_slab_plan.hip: use_ah), the column-stream planner for sv <= 1024 (smk_cols_plan.hip): at 2048 texels the two kernels
# take different paths for the same three-channel frame
WIDE = (2048, 4)
assert 1024 < WIDE[0] <= 2048


def tables(kind):
    """kind: '2d' first table alone; '2d3' + the two-axis third table; 'wide' the 2048 x 4 pair; '3d' the dense 3-D table.
    Returns (tf_mode, tf_vg, tf_h, tf3d)"""
    if kind == "2d":
        return 1, tf_ramp(), None, None
    if kind == "2d3":
        return 1, tf_ramp(), tf_third(), None
    if kind == "wide":
        return 1, tf_ramp(*WIDE), tf_third(*WIDE), None
    if kind == "3d":
        return 2, None, None, tf3d_dense()
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ scenes

def third_axis(mode, nelts, tf_h):
    """the rule: a third-axis data mode, at least three channels, a second table"""
    return 1 if (mode in THIRD and nelts >= 3 and tf_h is not None) else 0


def pose(sc, name):
    if name == "rot":
        sc.xform = O.rotation((1, 1, 0), 30)
    elif name == "close":                      # a close-up: the volume overflows the window on every side
        sc.xform = O.rotation((.3, 1, .2), 40)
        sc.eye = (0.05, -0.04, -1.6)
        sc.frustum = (-.25, .25, -.25, .25)
    else:
        sc.xform = O.rotation(*POSES[name])    # "x+" / "x-": a view along x (the x-major copy)


def scene(nelts, f32, table="2d", mode=None, shade=1, view="rot", window=WINDOWS[0], steps=48, dims=DIMS, grad=True,
          seed=3):
    """one case's checker scene; sc.dmode is the data mode the product is told, sc.tf_h is set whenever the case sets a
    second table -- whether the mode uses it or not: sc.third_axis says so"""
    data, nrm = layout(nelts, f32, dims, seed)
    sc = O.Scene(data, grad=nrm if grad else None)
    sc.tf_mode, sc.tf_vg, sc.tf_h, sc.tf3d = tables(table)
    sc.dmode = mode or DEFAULT_MODE[nelts]
    sc.third_axis = third_axis(sc.dmode, nelts, sc.tf_h)
    sc.width, sc.height = window
    sc.steps = steps
    sc.shade_mode = shade
    pose(sc, view)
    return sc


def with_data(sc, data, grad="same"):
    """the same frame set-up over other voxels (a zeroed or swapped channel, no normals)"""
    out = O.Scene(data, grad=sc.grad if isinstance(grad, str) else grad)
    for k, v in vars(sc).items():
        if k not in ("data", "grad", "dims", "nelts", "fsize", "region"):
            setattr(out, k, v)
    out.region = sc.region
    return out


# section a of test_gpu_layouts.py: (nelts, f32, table, shade, view, window); the data mode is DEFAULT_MODE's
def channel_cases():
    out = []
    views = ("rot", "x+", "close")
    for f32 in (False, True):
        for nelts in (1, 2, 3, 4):
            i = nelts + (4 if f32 else 0)
            out.append((nelts, f32, "2d" if nelts < 3 else "2d3", 1, views[i % 3], WINDOWS[i % 2]))
            if nelts >= 3:
                out.append((nelts, f32, "3d", 1, views[(i + 1) % 3], WINDOWS[(i + 1) % 2]))
        out.append((3, f32, "wide", 1, "rot", WINDOWS[0]))           # the planners part ways here (WIDE)
        out.append((4, f32, "wide", 2, "x-", WINDOWS[1]))            # NV20 shading, one case of each type
    return out


def case_id(c):
    nelts, f32, table, shade, view, window = c
    return "n%d-%s-%s-sh%d-%s-%dx%d" % (nelts, "f32" if f32 else "u8", table, shade, view, window[0], window[1])


def case_scene(c, **kw):
    nelts, f32, table, shade, view, window = c
    return scene(nelts, f32, table, shade=shade, view=view, window=window, steps=40 + 6 * nelts, **kw)


# ------------------------------------------------------------------------------------------------ bricks

# Brick boundaries per axis for the 21 x 13 x 7 volume, by grid.  Uneven on every axis that is cut, and placed against the
# boxes the shards keep (stored_box): rank 0 of 2 or 4 keeps x < 12 (u8; 11 for f32), the last rank x >= 9, so under
# (3, 1, 2) every rank has a brick wholly outside its box and one that straddles it; under (2, 2, 2) a single cut in x
# cannot lie outside both halves' boxes -- it is at 13, beyond rank 0's, and the y cut at 5 is below rank 3 of 4's
CUTS = {(1, 1, 1): ([0, 21], [0, 13], [0, 7]),
        (2, 2, 2): ([0, 13, 21], [0, 5, 13], [0, 3, 7]),
        (3, 1, 2): ([0, 6, 14, 21], [0, 13], [0, 4, 7])}


def cuts(dims, grid):
    if tuple(grid) == (1, 1, 1):
        return tuple([0, n] for n in dims)
    assert tuple(dims) == DIMS_ODD
    return CUTS[tuple(grid)]


def _f32_sum_to(total, pos):
    """a float32 size s with float32(pos + s) == total exactly: the product takes the volume's extent as the largest
    fPos + fSize over the bricks, and a bricked upload must see the extent the single brick states"""
    total, pos = np.float32(total), np.float32(pos)
    s = np.float32(total - pos)
    for _ in range(4):
        got = np.float32(pos + s)
        if got == total:
            return s
        s = np.nextafter(s, np.float32(np.inf if got < total else -np.inf), dtype=np.float32)
    raise AssertionError("no float32 size closes %r + s = %r" % (pos, total))


def bricks(dims, fsize, grid):
    """[(ipos, isize, fpos, fsize)] of the tiling cuts(dims, grid), x fastest; one brick for grid (1, 1, 1)"""
    cx, cy, cz = cuts(dims, grid)
    axes = (cx, cy, cz)
    out = []
    for k in range(len(cz) - 1):
        for j in range(len(cy) - 1):
            for i in range(len(cx) - 1):
                idx = (i, j, k)
                ipos = tuple(axes[a][idx[a]] for a in range(3))
                isize = tuple(axes[a][idx[a] + 1] - axes[a][idx[a]] for a in range(3))
                fpos, fs = [], []
                for a in range(3):
                    p = np.float32(np.float32(fsize[a]) * ipos[a] / dims[a])
                    if ipos[a] + isize[a] == dims[a]:
                        s = _f32_sum_to(fsize[a], p)
                    else:
                        s = np.float32(np.float32(fsize[a]) * isize[a] / dims[a])
                    fpos.append(float(p))
                    fs.append(float(s))
                out.append((ipos, isize, tuple(fpos), tuple(fs)))
    return out


def shuffled(n, seed=11):
    return [int(i) for i in np.random.default_rng(seed).permutation(n)]


def stored_box(dims, rank, nranks, u8, halo=1):
    """(origin, size) of the box a context keeps: its shard's region (sortlast.shard_region: bit 0 of the rank halves x,
    bit 1 y, bit 2 z) plus the halo, u8 rows made even in x and y by one more voxel where the volume has one, else by a
    pad column (include/smk.h, smk_set_shard)"""
    from simian_spacemonkey_amd import sortlast
    g0, g1 = sortlast.shard_region(dims, rank, nranks)
    o, d = [], []
    for a in range(3):
        lo, hi = max(g0[a] - halo, 0), min(g1[a] + halo, dims[a])
        if u8 and a < 2 and (hi - lo) & 1:
            if hi < dims[a]:
                hi += 1
            elif lo > 0:
                lo -= 1
            else:
                hi += 1        # the pad column, past the volume
        o.append(lo)
        d.append(hi - lo)
    return tuple(o), tuple(d)


def brick_relation(b, box):
    """'in', 'out' or 'cut': a brick against a stored box"""
    (ipos, isize, _, _), (o, d) = b, box
    inside = all(ipos[a] >= o[a] and ipos[a] + isize[a] <= o[a] + d[a] for a in range(3))
    apart = any(ipos[a] >= o[a] + d[a] or ipos[a] + isize[a] <= o[a] for a in range(3))
    return "out" if apart else "in" if inside else "cut"


def descriptors(data, grad, fsize, grid=(1, 1, 1), order=None, to_device=None):
    """(descriptor array, keep-alive list) of the volume cut into bricks(...), handed over in `order`; to_device: a function
    numpy array -> (device pointer, owner) for uploads from device memory"""
    from simian_spacemonkey_amd.binding import VolumeDesc      # smk_volume_desc (include/smk.h)
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


# ------------------------------------------------------------------------------------------------ the product's side

def upload(r, sc, grid=(1, 1, 1), order=None, to_device=None, timestep=None, stream=None, ready=None):
    """smk_upload_volume[_device] / smk_upload_timestep[_device] with the case's bricks and data mode, called directly: the
    binding's own helper cuts equal bricks in grid order.  ready: called once the bricks are made, before they are handed
    over (device bricks: wait for their copies).  Returns what keeps the bricks alive"""
    descs, keep = descriptors(sc.data, sc.grad, sc.fsize, grid, order, to_device)
    if ready is not None:
        ready()
    dt = 0 if sc.data.dtype == np.uint8 else 1
    mode = MODES.index(sc.dmode)
    if timestep is None:
        f = r.L.smk_upload_volume_device if to_device else r.L.smk_upload_volume
        rc = f(r.ctx, descs, len(descs), sc.nelts, dt, mode)
    elif to_device:
        rc = r.L.smk_upload_timestep_device(r.ctx, int(timestep), descs, len(descs), sc.nelts, dt, mode, stream)
    else:
        rc = r.L.smk_upload_timestep(r.ctx, int(timestep), descs, len(descs), sc.nelts, dt, mode)
    r._ck(rc)
    return keep


def frame_state(r, sc):
    """everything of a frame but the volume (the draw() part of _scenes.push_scene); the second table is handed over
    whenever the case has one: whether it is used is the product's decision, by the data mode"""
    r.set_option("tf_raw", 1)
    if sc.tf_mode == 1:
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


def push(r, sc, grid=(1, 1, 1), order=None, do_upload=True):
    if do_upload:
        upload(r, sc, grid, order)
    frame_state(r, sc)


# ------------------------------------------------------------------------------------------------ the slice quad

def _model_from_eye(sc, pts):
    """eye-space points -> model space (the units of fPos / fSize) under the scene's modelview"""
    M = np.array(sc.mv(), np.float64).reshape(4, 4).T
    Mi = np.linalg.inv(M)
    return (Mi[:3, :3] @ np.asarray(pts, np.float64).T).T + Mi[:3, 3]


def _eye_from_model(sc, pts):
    M = np.array(sc.mv(), np.float64).reshape(4, 4).T
    return (M[:3, :3] @ np.asarray(pts, np.float64).T).T + M[:3, 3]


def quads(sc):
    """the slice quads of a scene, name -> 4 x 3 in model space; the last three must draw nothing"""
    fs = np.array([float(f) for f in sc.fsize])
    nz = sc.dims[2]
    q = {}
    ob = np.array([[0.1, 0.15, 0.3], [0.9, 0.1, 0.35], [0.85, 0.9, 0.6], [0.15, 0.8, 0.55]])
    ob[3] = ob[0] + (ob[2] - ob[1])                       # exactly planar
    q["oblique"] = ob * fs
    zc = (nz // 2 + 0.5) / nz                             # a voxel-centre plane
    q["axis"] = np.array([[.08, .1, zc], [.93, .1, zc], [.93, .88, zc], [.08, .88, zc]]) * fs
    out = np.array([[-.45, -.4, .2], [1.4, -.4, .35], [1.4, 1.5, .8], [-.45, 1.5, .65]])
    out[3] = out[0] + (out[2] - out[1])
    q["outside"] = out * fs                               # texture coordinates far outside [0, 1]: clamp to edge
    cen = _eye_from_model(sc, [fs / 2])[0]
    # seen nearly edge-on: spanned by the window's x and a direction six degrees off the line of sight
    los = cen / np.linalg.norm(cen)
    u = np.array([.42, 0, 0])
    v = .45 * (np.sin(np.deg2rad(6)) * np.array([0, 1, 0]) + np.cos(np.deg2rad(6)) * los)
    q["edge_on"] = _model_from_eye(sc, [cen - u - v, cen + u - v, cen + u + v, cen - u + v])
    # wholly behind the eye: the oblique quad mirrored through the eye point (its rays would hit it at t < 0)
    q["behind"] = _model_from_eye(sc, -_eye_from_model(sc, q["oblique"]))
    a, b = q["oblique"][0], q["oblique"][2]
    q["zero_area"] = np.array([a, a + .3 * (b - a), a + .7 * (b - a), b])     # four points of one line
    e = _eye_from_model(sc, q["oblique"])
    e[:, 0] += 1.5 * abs(cen[2]) * (sc.frustum[1] - sc.frustum[0]) / sc.znear  # one and a half windows to the right
    q["off_screen"] = _model_from_eye(sc, e)
    return {k: np.ascontiguousarray(v, np.float64) for k, v in q.items()}


NO_DRAW = ("behind", "zero_area", "off_screen")
ALPHAS = (0.0, 0.6, 2.5)
# (window, quad): every quad at 37 x 29; at 16 x 16 -- one tile of the kernel exactly -- the quads whose outline the
# reference alone keeps under the edge cap there (test_layouts_cpu.py checks it for every pair listed)
SLICE_CASES = tuple(((37, 29), q) for q in ("oblique", "axis", "outside", "edge_on") + NO_DRAW) + \
    tuple(((16, 16), q) for q in ("outside", "edge_on") + NO_DRAW)


def slice_scene(nelts, f32, window=(37, 29), seed=3):
    """a scene for the slice quad: make_vgh leaves the outermost voxels of the first three channels at 0, under which a
    clamped fetch outside the box -- or a quad drawn where none should be -- adds nothing and could not show; channel 0
    here is the mean of the value and the fourth field, which reaches the faces.  The other channels are as in layout()"""
    u8, f, nrm = _four(tuple(DIMS), seed)
    if f32:
        data = f[..., :nelts].copy()
        data[..., 0] = (f[..., 0] + f[..., 3]) * np.float32(.5)
    else:
        data = u8[..., :nelts].copy()
        data[..., 0] = (u8[..., 0].astype(np.uint16) + u8[..., 3]) // 2
    sc = O.Scene(data, grad=nrm)
    sc.tf_mode, sc.tf_vg, sc.tf_h, sc.tf3d = tables("2d")
    sc.dmode = DEFAULT_MODE[nelts]
    sc.width, sc.height = window
    sc.steps = 40
    sc.shade_mode = 0
    pose(sc, "rot")
    return sc


def slice_reference(sc, base, quad, alpha):
    """(frame, edge mask): gl_slices.render_quad_slice of channel 0 in float64 over `base`"""
    import gl_slices
    want = np.array(base, np.float64)
    vol = sc.data[..., 0].astype(np.float64)
    if sc.data.dtype == np.uint8:
        vol = vol / 255.0
    edge = gl_slices.render_quad_slice(want, vol, sc.fsize, sc.mv(), sc.frustum, sc.znear, 20.0, quad, alpha)
    return want, edge


# ------------------------------------------------------------------------------------------------ the other sections' cases

RULE_VOLUMES = (3, 4)                      # u8 channel counts rendered under all 13 data modes with a second table


def rule_scene(nelts, mode, second=True):
    return scene(nelts, False, "2d3" if second else "2d", mode=mode, shade=1, view="rot", steps=44)


def no_normals_scene(f32):
    return scene(3, f32, "2d3", shade=1, view="rot", grad=False, steps=44)


PACK_LAYOUTS = ((1, False), (3, False), (4, False), (2, True), (4, True))      # (nelts, f32), all at 21 x 13 x 7
PACK_GRIDS = ((2, 2, 2), (3, 1, 2))
PACK_SHARDS = ((0, 1), (0, 2), (1, 2), (0, 4), (3, 4))                          # (rank, nranks)


def pack_scene(nelts, f32):
    return scene(nelts, f32, "2d" if nelts < 3 else "2d3", shade=1, view="rot", dims=DIMS_ODD, steps=40)


def step_scenes():
    """two four-channel f32 time steps with different data and different normals"""
    return [scene(4, True, "2d3", shade=1, view="rot", steps=44, seed=s) for s in (3, 4)]


SHADOW = (96, 0.5)                         # light buffer and quality of test_host_adapter.py's shadow tests
SHADOW_LIGHT = (3, 4, -3)                  # test_gpu_shadow.py's "oblique"


def shadow_scene(f32):
    sc = scene(4, f32, "2d3", shade=1, view="rot", steps=48)
    sc.light_pos = SHADOW_LIGHT
    sc.shadow = SHADOW
    return sc


def wide_range_scene():
    """three-channel f32 voxels scaled to about [-0.3, 1.3]: the table lookups clamp, the trilinear fetch does not"""
    sc = scene(3, True, "2d3", shade=1, view="rot", steps=44)
    return with_data(sc, (sc.data * np.float32(1.6) - np.float32(.3)).astype(np.float32))
