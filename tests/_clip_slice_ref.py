"""The clip-plane widget's data slice (smk.h smk_set_clip_slice) restated from the reference, float64 numpy.

TEST INFRASTRUCTURE ONLY.  Written from drawClip / renderSlice of the two live renderers, not from the HIP kernel:

  * when (R8kVolRen3D.cpp:360-372, 400-424; NV20VolRen3D.cpp:144-148, 173-178): drawClip(dv) before the volume's slices,
    drawClip(-dv) after them; its switch over gluvv.clip.oaxis (R8kVolRen3D.cpp:826-879) draws when
        X+ dv < 0, X- dv > 0 (no range test), Y+ dv > 0, Y- dv < 0, Z+ dv < 0, Z- dv > 0
    and corner 0's clamped coordinate on the axis lies strictly inside (0, fSize); with shadows the before pass needs
    axis[3] = vdl <= 0 (:306-324, 360);
  * where (:810-823, 906-913): the corners clamped to the (sub-)volume's box in float, moved by +-0.001 along the axis,
    one GL_QUADS quad = triangles (0, 1, 2), (0, 2, 3), texture coordinates = the moved vertex / fSize;
  * colour: the R8k clip shader createFragClip (:3190-3250) over the texture createBricks makes of the data mode
    (:1926-2055; loadTex1B GL_ALPHA8, loadTex2B GL_LUMINANCE8_ALPHA8, loadTex4B GL_RGBA8) or the NV20 final combiner
    (NV20VolRen3D.cpp:390, 426-431);
  * order (GL_ONE, GL_ONE_MINUS_SRC_ALPHA, :364, 404, 416), onto the volume layer V of a cleared frame:
    before  V + (1 - V.a) src  (max(V, src) under GL_MAX, NV20VolRen3D.cpp:144-163),  after  src + (1 - src.a) V;
  * depth test on, depth writes off (:365, 405, 417): a slice pixel exists where its view depth is LESS than the scene's.

A pixel is covered where the ray through its centre meets one of the two triangles (what GL's rasteriser decides with
perspective-correct interpolation: the texture coordinate IS the hit point / fSize).  `dtype` lets the coverage decision be
repeated in float32 (the tests check that their poses do not hinge on it).
"""
import numpy as np

THIRD_AXIS = ("VGH", "V1GH", "V2G", "V2GH", "V3", "V3G", "V4")      # createFragClip's switch (:3193-3208)
TWO_BYTE = ("V1G", "V2", "VGH_VG")                                  # createBricks (:1969-1971)
ONE_BYTE = ("V1", "VGH_V")                                          # (:1950-1951)
OFFSET = np.float32(.001)                                           # (:823)


def clamped_corners(corners, fsize):
    """CLAMP_ARB(0, c - fPos, fSize) of the whole volume (fPos = 0), in float as the reference computes it"""
    c = np.array(corners, np.float32).reshape(4, 3)
    fs = np.array([np.float32(f) for f in fsize], np.float32)
    return np.minimum(np.maximum(c, np.float32(0)), fs)


def _case(oaxis, d, c0, fs):
    inside = (c0 > 0) and (c0 < fs)
    return {1: d < 0 and inside, 2: d > 0, 3: d > 0 and inside, 4: d < 0 and inside, 5: d < 0 and inside,
            6: d > 0 and inside}[oaxis]


def pass_rule(oaxis, dv, corners, fsize, vdl=None):
    """0 none, 1 before the volume, 2 after it.  vdl: the shadow mode's dot(light direction, view axis), None without shadows"""
    c = clamped_corners(corners, fsize)
    a = (oaxis - 1) // 2
    c0, fs = float(c[0, a]), float(np.float32(fsize[a]))
    if _case(oaxis, dv, c0, fs) and (vdl is None or vdl <= 0):
        return 1
    if _case(oaxis, -dv, c0, fs):
        return 2
    return 0


def moved_quad(corners, fsize, oaxis):
    """the four vertices renderSlice receives: clamped, then moved along the axis (float arithmetic, addV3)"""
    c = clamped_corners(corners, fsize)
    a = (oaxis - 1) // 2
    c[:, a] = c[:, a] + (OFFSET if (oaxis - 1) % 2 == 0 else -OFFSET)
    return c


def _rays(mv, frustum, znear, width, height, dtype):
    """origin and per-pixel direction (model space) of the rays through the pixel centres; a point o + t d has view depth t"""
    M = np.array(mv, np.float64).reshape(4, 4).T
    inv = np.linalg.inv(M)
    l, r, b, t = [float(v) for v in frustum]
    px = l + (np.arange(width, dtype=np.float64) + .5) * (r - l) / width
    py = b + (np.arange(height, dtype=np.float64) + .5) * (t - b) / height
    de = np.stack(np.broadcast_arrays(px[None, :] / znear, py[:, None] / znear, -np.ones((height, width))), axis=-1)
    d = de @ inv[:3, :3].T
    return inv[:3, 3].astype(dtype), d.astype(dtype)


def intersect(quad, mv, frustum, znear, width, height, dtype=np.float64):
    """(cover [H][W] bool, hit [H][W][3] model space, depth [H][W]) of the quad's two triangles, first triangle first"""
    q = np.array(quad, np.float64).astype(dtype)
    o, d = _rays(mv, frustum, znear, width, height, dtype)
    cover = np.zeros((height, width), bool)
    hit = np.zeros((height, width, 3), dtype)
    depth = np.full((height, width), np.inf, dtype)
    for k in (1, 2):
        v0, e1, e2 = q[0], q[k] - q[0], q[k + 1] - q[0]
        pv = np.cross(d, e2)
        det = pv @ e1
        tv = o - v0
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (pv @ tv) / det
            qv = np.cross(tv, e1)
            w = (d @ qv) / det
            tt = (e2 @ qv) / det
        ok = (det != 0) & (u >= 0) & (w >= 0) & (u + w <= 1) & (tt > 0) & ~cover
        hit[ok] = (v0 + u[..., None] * e1 + w[..., None] * e2)[ok]
        depth[ok] = tt[ok]
        cover |= ok
    return cover, hit, depth


def edge_pixels(quad, mv, frustum, znear, zfar, width, height, tol=1e-3):
    """pixels whose centre lies within `tol` pixels of one of the projected quad's four edges"""
    M = np.array(mv, np.float64).reshape(4, 4).T
    q = np.array(quad, np.float64)
    eye = q @ M[:3, :3].T + M[:3, 3]
    l, r, b, t = [float(v) for v in frustum]
    w = -eye[:, 2]
    win = np.stack([(eye[:, 0] * znear / w - l) / (r - l) * width, (eye[:, 1] * znear / w - b) / (t - b) * height], axis=1)
    X, Y = np.meshgrid(np.arange(width) + .5, np.arange(height) + .5)
    P = np.stack([X, Y], axis=-1)
    near = np.zeros((height, width), bool)
    for k in range(4):
        a, c = win[k], win[(k + 1) % 4]
        ab = c - a
        s = np.clip(((P - a) @ ab) / max(ab @ ab, 1e-300), 0, 1)
        dist = np.linalg.norm(P - (a + s[..., None] * ab), axis=-1)
        near |= dist < tol
    return near


def _fetch(tex, tc):
    """GL_LINEAR, GL_CLAMP_TO_EDGE of tex[z][y][x][ch] at texture coordinates tc[..., 3] (s, t, r)"""
    nz, ny, nx = tex.shape[:3]
    idx = []
    for c, n in ((tc[..., 0], nx), (tc[..., 1], ny), (tc[..., 2], nz)):
        u = np.clip(c * n - .5, 0, n - 1.0)
        i0 = np.minimum(np.floor(u).astype(np.int64), max(n - 2, 0))
        idx.append((i0, np.minimum(i0 + 1, n - 1), u - i0))
    (x0, x1, fx), (y0, y1, fy), (z0, z1, fz) = idx
    out = 0
    for zi, wz in ((z0, 1 - fz), (z1, fz)):
        for yi, wy in ((y0, 1 - fy), (y1, fy)):
            for xi, wx in ((x0, 1 - fx), (x1, fx)):
                out = out + (wz * wy * wx)[..., None] * tex[zi, yi, xi]
    return out


def data_texture(data, dmode):
    """the RGBA texels (float64; u8 data / 255, f32 data as it is) createBricks' texture returns for the data mode"""
    d = np.asarray(data)
    v = d.astype(np.float64) / 255.0 if d.dtype == np.uint8 else d.astype(np.float64)
    ne = d.shape[-1]
    zero = np.zeros(d.shape[:3])
    if dmode in ONE_BYTE:                                   # GL_ALPHA8
        ch = [zero, zero, zero, v[..., 0]]
    elif dmode in TWO_BYTE:                                 # GL_LUMINANCE8_ALPHA8
        ch = [v[..., 0], v[..., 0], v[..., 0], v[..., 1]]
    elif dmode in THIRD_AXIS:                               # GL_RGBA8, alpha 50 where the data has three elements (:2003)
        ch = [v[..., 0], v[..., 1], v[..., 2], v[..., 3] if ne > 3 else zero + 50.0 / 255.0]
    else:
        raise ValueError(dmode)
    return np.stack(ch, axis=-1)


def sat(x):
    return np.clip(x, 0.0, 1.0)


def shade(texel, alpha, look, dmode):
    """src RGBA (premultiplied) of interpolated texels"""
    if look == "nv20":      # final combiner: rgb = tex * const0.a, alpha = const0.a; the value channel
        v = sat(texel[..., 0] if dmode not in ONE_BYTE else texel[..., 3])
        return np.stack([v * alpha, v * alpha, v * alpha, np.full(v.shape, float(alpha))], axis=-1)
    rgb = texel[..., :3].copy()
    if dmode not in THIRD_AXIS:
        rgb[..., 1] = texel[..., 3]     # MOV r0.g <- r0.a
    rgb = sat(rgb)
    a = float(sat(alpha))
    return np.concatenate([sat(rgb * a), np.full(rgb.shape[:-1] + (1,), a)], axis=-1)


def slice_layer(data, dmode, fsize, mv, frustum, znear, width, height, corners, oaxis, alpha, look, scene_depth=None):
    """(S [H][W][4] float64 -- zero where the quad does not cover --, cover, view depth) of the slice the reference draws;
    scene_depth: [H][W] VIEW depths, the GL_LESS test in float as the product compares (+inf / NaN: no occluder)"""
    quad = moved_quad(corners, fsize, oaxis)
    cover, hit, depth = intersect(quad, mv, frustum, znear, width, height)
    if scene_depth is not None:
        zs = np.where(np.isnan(scene_depth), np.inf, scene_depth).astype(np.float32)
        cover = cover & (depth.astype(np.float32) < zs)
    fs = np.array([float(np.float32(f)) for f in fsize])
    S = np.zeros((height, width, 4))
    if cover.any():
        texel = _fetch(data_texture(data, dmode), hit[cover] / fs)
        S[cover] = shade(texel, alpha, look, dmode)
    return S, cover, depth


def compose(V, S, cover, pass_, blend_max=False):
    """the frame of a volume layer V and the slice layer S drawn in pass 1 (before) or 2 (after); 0: V"""
    out = np.array(V, np.float64)
    if pass_ == 0:
        return out
    v, s = out[cover], S[cover]
    if pass_ == 1:
        out[cover] = np.maximum(v, s) if blend_max else v + (1 - v[..., 3:4]) * s
    else:
        out[cover] = s + (1 - s[..., 3:4]) * v
    return out
