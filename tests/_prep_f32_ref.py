"""NumPy float32 restatement of the float data-preparation contracts (include/smk.h: smk_normals_f32_device,
smk_merge_fields_f32_device, smk_hist2d_f32_device), vectorised, no GPU.

The library is built without floating-point contraction and every step of the contracts is one fp32 operation, so
the arrays below are what the kernels must produce bit for bit.  tests/test_prep_f32_ref.py ties this module to the
reference-derived checker on byte data; tests/test_gpu_prep_f32.py holds the kernels to it.

Volumes are [z][y][x][channels] float32.
"""
import math

import numpy as np

F = np.float32
_IGNORE = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")


def central_differences(ch):
    """g[z][y][x][3] of one channel [z][y][x]: d[o + stride_e] - d[o - stride_e], one fp32 subtraction, 0 on the border"""
    ch = np.asarray(ch, F)
    g = np.zeros(ch.shape + (3,), F)
    with np.errstate(**_IGNORE):
        g[1:-1, 1:-1, 1:-1, 0] = ch[1:-1, 1:-1, 2:] - ch[1:-1, 1:-1, :-2]
        g[1:-1, 1:-1, 1:-1, 1] = ch[1:-1, 2:, 1:-1] - ch[1:-1, :-2, 1:-1]
        g[1:-1, 1:-1, 1:-1, 2] = ch[2:, 1:-1, 1:-1] - ch[:-2, 1:-1, 1:-1]
    return g


def blur_gradient(g):
    """blurV3D as the kernels gather it: the 27 sources in ascending (dz, dy, dx) order, weight by the number of
    non-zero offsets, a = a + w * s, then one division.  Border and outside sources hold the zero gradient."""
    w = (F(1.0), F(.3), F(.2), F(.1))
    nz, ny, nx = g.shape[:3]
    p = np.pad(g, ((1, 1), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros_like(g)
    with np.errstate(**_IGNORE):
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                for dk in (-1, 0, 1):
                    src = p[1 + di:1 + di + nz, 1 + dj:1 + dj + ny, 1 + dk:1 + dk + nx]
                    acc = acc + w[(di != 0) + (dj != 0) + (dk != 0)] * src
        div = F(1.0) + F(6) * F(.3) + F(12) * F(.2) + F(8) * F(.1)
        return acc / div


def normal_bytes(g):
    """scalebiasN with the +1 -> 255 clamp; a gradient with a component that is not finite gives (128, 128, 128)"""
    g = np.asarray(g, F)
    fin = np.isfinite(g).all(axis=-1)
    g = np.where(fin[..., None], g, F(0))
    with np.errstate(**_IGNORE):
        ln = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2])
        pos = ln > 0
        n = np.where(pos[..., None], g / np.where(pos, ln, F(1))[..., None], g)
        s = n * F(128) + F(128)
    assert s.dtype == F
    out = np.where(s >= F(255), 255, s.astype(np.int32) & 0xff).astype(np.uint8)
    out[~fin] = 128
    return out


def normals_f32(vol, blur=False):
    """smk_normals_f32_device: the normal bytes [z][y][x][3] of channel 0's gradient"""
    g = central_differences(np.asarray(vol, F)[..., 0])
    if blur:
        g = blur_gradient(g)
    return normal_bytes(g)


def merge_fields_f32(fields):
    """smk_merge_fields_f32_device: (out [z][y][x][nf+1] f32, normals [z][y][x][3] u8)"""
    fields = np.ascontiguousarray(fields, F)
    nf = fields.shape[-1]
    g = np.zeros(fields.shape[:3] + (3,), F)
    with np.errstate(**_IGNORE):
        for e in range(nf):
            g = g + central_differences(fields[..., e])
        mag = np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2])
        fin = np.isfinite(mag)
        maxm = mag[fin].max() if fin.any() else F(0)
        G = np.where(fin & (maxm > 0), mag / (maxm if maxm > 0 else F(1)), F(0)).astype(F)
    assert mag.dtype == F
    out = np.empty(fields.shape[:3] + (nf + 1,), F)
    out.view(np.uint32)[..., :nf] = fields.view(np.uint32)
    out[..., nf] = G
    return out, normal_bytes(g)


def hist_bin(v):
    """a channel's bin: t = v * 255 in fp32; NaN or t < 0 -> 0, t >= 255 -> 255, otherwise (int)t"""
    with np.errstate(**_IGNORE):
        t = np.asarray(v, F) * F(255.0)
        mid = (t >= 0) & (t < F(255))
        b = np.where(mid, t, F(0)).astype(np.int32)
    b[t >= F(255)] = 255
    return b.astype(np.uint8)


def hist_finish(counts):
    """the reference's log-scaled bytes of 65536 counts: float bins that stop at 2^24, h = (float)log(count),
    hist = (uchar)(h / max * 255), 0 for an empty bin and when no bin holds more than one voxel"""
    ih = np.minimum(np.asarray(counts, np.int64), 1 << 24)
    u, inv = np.unique(ih, return_inverse=True)    # (libm's log, as the library and the checker call it)
    lg = np.array([math.log(float(c)) if c > 0 else -np.inf for c in u], F)[inv.ravel()]
    mx = max(F(0), lg.max())
    hist = np.zeros(65536, np.uint8)
    if mx > 0:
        ok = np.isfinite(lg)
        hist[ok] = (lg[ok] / F(mx) * F(255)).astype(np.int32).astype(np.uint8)
    return hist.reshape(256, 256)


def hist2d_f32(vol):
    """smk_hist2d_f32_device: hist[b(c1)][b(c0)] of a volume with at least two channels"""
    vol = np.asarray(vol, F)
    assert vol.shape[-1] >= 2
    key = hist_bin(vol[..., 1]).astype(np.int64).ravel() * 256 + hist_bin(vol[..., 0]).ravel()
    return hist_finish(np.bincount(key, minlength=65536))
