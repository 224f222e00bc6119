"""The opacity correction of the 2-D table (option "tf_raw" 0, the product's default) restated in plain numpy float64,
for the tests that compare what the device kernel wrote with something the product did not compute itself.

The map is NV20VolRen3D::copyScale's (:1645-1660): alpha byte a becomes floor((1 - (1 - a/255)^(1/rate)) * 255), the
exponent rounded to float32 as copyScale's `float alphaScale` is.  The rate is include/smk.h's (smk_set_sampling):
sample_rate / gamma, in steps mode fsize[0] / (N[0] * dis) / gamma with dis the view-depth extent / steps -- taken
here from the CPU checker's ray set-up, never from the product; without scale_alphas it is 1 / gamma."""
import numpy as np

from _scenes import push_scene


def alpha_map(sr):
    """copyScale per possible alpha byte: uint8 [256]"""
    s = float(np.float32(1.0 / float(np.float32(sr))))
    a = np.arange(256, dtype=np.float64)
    return np.floor((1.0 - (1.0 - a / 255.0) ** s) * 255.0).astype(np.uint8)


def apply(raw, sr):
    """the effective table: `raw` [sg][sv][4] uint8 with the map applied to its alpha channel"""
    out = np.array(raw, dtype=np.uint8, copy=True)
    out[..., 3] = alpha_map(sr)[out[..., 3]]
    return out


def frame_rate(sc, gamma=1.0, scale_alphas=1):
    """the correction rate of the checker scene's frame as smk.h documents it (a float32)"""
    if not scale_alphas:
        return np.float32(1) / np.float32(gamma)
    if sc.steps > 0:
        dis = sc.raycoef().dis
        rate = np.float32(float(np.float32(sc.fsize[0])) / (float(sc.dims[0]) * float(dis)))
    else:
        rate = np.float32(sc.sample_rate)
    return rate / np.float32(gamma)


def push_corrected(r, sc, raw, gamma=1.0, scale_alphas=1, grid=(1, 1, 1), upload=True):
    """push_scene, then hand the product the RAW table and let it correct it on the device; the checker scene gets the
    table this module corrected.  Returns the rate."""
    sc.tf_vg = np.ascontiguousarray(raw, np.uint8)
    push_scene(r, sc, grid, upload=upload)
    r.set_option("tf_raw", 0)
    r.set_tf2d(raw, sc.tf_h if sc.third_axis else None)
    r.set_sampling(sc.sample_rate, sc.steps, gamma, scale_alphas)
    rate = frame_rate(sc, gamma, scale_alphas)
    sc.tf_vg = apply(raw, rate)
    return rate


def ramp_table(sv, sg, seed=7):
    """a table that uses every alpha byte (at 256 x 256): alpha s * 255 // (sv - 1) along v, scaled per row by
    (16 - (t + 5) % 8) / 16 (row 0: 11 / 16, so that a one-row table has alphas the correction moves), over it -- from 16
    columns up -- one band of columns with alpha 1-2 only (what a rate above 1 truncates to zero) and one with alpha 255;
    seeded colours"""
    rng = np.random.default_rng(seed)
    tex = np.zeros((sg, sv, 4), np.uint8)
    tex[..., :3] = rng.integers(32, 256, (sg, sv, 3))
    s = np.arange(sv)[None, :]
    t = np.arange(sg)[:, None]
    tex[..., 3] = (s * 255 // (sv - 1)) * (16 - (t + 5) % 8) // 16
    if sv >= 16:
        lo, hi = low_band(sv), high_band(sv)
        tex[:, lo[0]:lo[1], 3] = (1 + ((s + t) & 1))[:, lo[0]:lo[1]]
        tex[:, hi[0]:hi[1], 3] = 255
    return tex


def low_band(sv):
    """[first, last + 1) columns of ramp_table's alpha 1-2 band"""
    return sv * 9 // 32, sv * 11 // 32 + 1


def high_band(sv):
    return sv * 20 // 32, sv * 22 // 32 + 1
