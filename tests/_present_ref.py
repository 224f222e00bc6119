"""The present rule (include/smk.h "display-ready frames") restated in numpy: what smk_present_device must produce, byte
for byte.  Colour in float32, one rounded operation per line (the library is built without fma contraction); depth in
float64, rounded to float32 once."""
import numpy as np

F = np.float32


def quantise(x):
    """q(x) = (uint8) floor(sat(x) * 255 + 0.5), NaN -> 0"""
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore"):
        x = np.where(x > F(0), x, F(0))        # NaN and -0.0 fail the comparison
        x = np.where(x < F(1), x, F(1))
    s = (x * F(255)).astype(F)
    r = (s + F(0.5)).astype(F)
    return np.floor(r).astype(np.uint8)


def present_rgba8(frame, bg=None):
    """frame [..., 4] premultiplied float RGBA -> [..., 4] uint8.  bg None: every channel through q.  bg = (r, g, b): the
    opaque colour under the frame, rgb = q(C + (1 - A) * b), a = 255"""
    frame = np.asarray(frame, F)
    if bg is None:
        return quantise(frame)
    b = np.asarray(bg, F)
    out = np.empty(frame.shape, np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (F(1) - frame[..., 3]).astype(F)
        for k in range(3):
            u = (t * b[k]).astype(F)
            out[..., k] = quantise((frame[..., k] + u).astype(F))
    out[..., 3] = 255
    return out


def window_depth(d, n, f):
    """view depth d (float32; +inf = nothing hit) -> float32 window depth z_w = f (d - n) / ((f - n) d), clamped to [0, 1];
    +inf and NaN give exactly 1, d <= n gives 0.  (n, f): the camera's clip planes as float32 values"""
    d = np.asarray(d, F).astype(np.float64)
    n, f = np.float64(F(n)), np.float64(F(f))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        zw = (f * (d - n)) / ((f - n) * d)
        zw = np.where(zw < 0.0, 0.0, zw)
        zw = np.where(zw > 1.0, 1.0, zw)
        zw = np.where(d <= n, 0.0, zw)
        zw = np.where(d < np.inf, zw, 1.0)     # +inf, NaN
    return zw.astype(F)


def view_depth(zw, n, f):
    """INTEGRATION.md's inverse (smk_render_occluded's SMK_SCENE_WINDOW_DEPTH conversion), float64"""
    zw = np.asarray(zw, np.float64)
    n, f = np.float64(F(n)), np.float64(F(f))
    return f * n / (f - zw * (f - n))


def edge_values():
    """float32 values every test frame holds: the quantiser's edges, and each k/255 nudged by one ulp either way"""
    k = (np.arange(256, dtype=F) / F(255)).astype(F)
    special = np.array([0.0, -0.0, 1.0, 0.5, -1.0, 1.5, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e-39, 1.1754944e-38,
                        0.5 / 255, 254.5 / 255, 0.999999, 1.0000001], F)
    return np.concatenate([special, k, np.nextafter(k, F(2)), np.nextafter(k, F(-1))]).astype(F)
