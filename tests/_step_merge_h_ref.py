"""NumPy float32 restatement of the merge with H and blurred normals (include/smk.h: smk_merge_fields_h_device,
smk_merge_fields_h_f32_device, smk_merge_timestep_h, smk_upload_timestep_fields_h_device), and the volumes of
tests/test_gpu_step_merge_h.py.  No GPU; tests/test_step_merge_h_cpu.py qualifies both.

Every step of the contract is one fp32 operation on float32 arrays (one rounding each, in the order written); the two
affine maps of the H scaling run in float64; the byte cast is x86's (truncation through int32, 0 when out of range or NaN).

Volumes are [z][y][x][nf]; dims are (nx, ny, nz)."""
import numpy as np

import _prep_f32_ref as P
import _step_merge_ref as M
import _u16_ref as U

F32 = np.float32
_IGNORE = dict(invalid="ignore", over="ignore", under="ignore", divide="ignore")
TILE = (32, 8, 8)                      # MH_TX, MH_TY, MH_TZ (csrc/smk_step_merge_h.hip), in voxels (x, y, z)
STATS_BLOCKS = 2048                    # MH_STATS_BLOCKS: pass 1's grid is capped there and strides over the tiles
RINGS, NP, CODE, RING_OF = M.RINGS, M.NP, M.CODE, M.RING_OF
MODE = {(1, 0): "V1G", (2, 0): "V2G", (3, 0): "V3G", (1, 1): "V1GH", (2, 1): "V2GH"}   # (nf, add_h) -> the data mode


# ---- the contract

def summed(Ff):
    """S [z][y][x][3] of float fields"""
    return M.central_sum(np.ascontiguousarray(Ff, F32))


def second_derivative(S, compat):
    """hs [z][y][x]: gh_from_grads of S and S at the six neighbours at interior voxels (NaN where the gradient vanishes),
    0 on the border"""
    hs = np.zeros(S.shape[:3], F32)
    c = (slice(1, -1),) * 3
    g = [S[c + (a,)] for a in range(3)]
    xp, xm = S[1:-1, 1:-1, 2:], S[1:-1, 1:-1, :-2]
    yp, ym = S[1:-1, 2:, 1:-1], S[1:-1, :-2, 1:-1]
    zp, zm = S[2:, 1:-1, 1:-1], S[:-2, 1:-1, 1:-1]
    with np.errstate(**_IGNORE):
        gm = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        h = [p[..., a] - m[..., a] for a in range(3) for p, m in ((xp, xm), (yp, ym), (zp, zm))]
        tg = [g[a] / gm for a in range(3)]
        tv0 = tg[0] * h[0] + tg[1] * h[1] + tg[2] * h[2]
        tv1 = (tg[0] * h[3] + tg[1] + tg[2] * h[5]) if compat else (tg[0] * h[3] + tg[1] * h[4] + tg[2] * h[5])
        tv2 = tg[0] * h[6] + tg[1] * h[7] + tg[2] * h[8]
        inner = tg[0] * tv0 + tg[1] * tv1 + tg[2] * tv2
    assert inner.dtype == F32
    hs[c] = inner
    return hs


def _ordered(f):
    i = np.ascontiguousarray(f, F32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, i ^ 0x7fffffff)


def _unordered(i):
    return np.array([i if i >= 0 else i ^ 0x7fffffff], np.int64).astype(np.int32).view(F32)[0]


def h_extremes(hs, flt):
    """(hmin, hmax) over the interior voxels from the seeds +1e8 / -1e8, as the ordered-integer atomics take them (-0 < +0);
    a NaN never wins, in the float pipeline nothing that is not finite does"""
    v = hs[1:-1, 1:-1, 1:-1]
    v = v[np.isfinite(v) if flt else ~np.isnan(v)]
    hmin, hmax = F32(1e8), F32(-1e8)
    if v.size:
        o = _ordered(v)
        lo, hi = _unordered(int(o.min())), _unordered(int(o.max()))
        hmin = hmin if hmin < lo else lo
        hmax = hmax if hi < hmax else hi
    return F32(hmin), F32(hmax)


def _affine(i, x, I, o, O):
    with np.errstate(**_IGNORE):
        return (np.float64(O) - np.float64(o)) * (np.asarray(x, np.float64) - np.float64(i)) / (np.float64(I) - np.float64(i)) + np.float64(o)


def uc_cast(x):
    x = np.asarray(x, np.float64)
    ok = (x > -2147483649.0) & (x < 2147483648.0)
    return (np.where(ok, x, 0.0).astype(np.int64) & 0xff).astype(np.uint8)


def h_scaled(hs, hmin, hmax):
    """vgh_scale's H of every voxel: (the double hq, its byte, its float with NaN -> 0)"""
    neg = hs < 0
    with np.errstate(**_IGNORE):
        th_n = _affine(hmin, hs, 0, 0, 1).astype(F32)
        th_p = _affine(0, hs, hmax, 0, 1).astype(F32)
        hq = np.where(neg, _affine(0, th_n, 1, 0, 255 // 3), _affine(0, th_p, 1, 255 // 3, 255 // 3 * 2))
        f = np.where(np.isnan(hq), 0.0, hq / 255.0).astype(F32)
    return hq, uc_cast(hq), f


def merge_h(F, add_h=1, compat=1, blur=0):
    """(data [z][y][x][nf + 1 + add_h] of the fields' type, normals [z][y][x][3] u8) of the fields F (u8, u16 or f32) in a
    ring of F's type"""
    F = np.ascontiguousarray(F)
    ring = RING_OF[F.dtype]
    flt = ring != "u8"
    nf = F.shape[-1]
    S = summed(F.astype(F32))
    with np.errstate(**_IGNORE):
        mag = np.sqrt(S[..., 0] * S[..., 0] + S[..., 1] * S[..., 1] + S[..., 2] * S[..., 2])
        inner = mag[1:-1, 1:-1, 1:-1]
        if flt:
            fin = inner[np.isfinite(inner)]
            maxm = F32(max(F32(0), fin.max())) if fin.size else F32(0)
            G = np.where(np.isfinite(mag) & (maxm > 0), mag / (maxm if maxm > 0 else F32(1)), F32(0)).astype(F32)
        else:
            maxm = F32(max(F32(0), inner.max()))
            G = uc_cast((mag / maxm).astype(F32).astype(np.float64) * 255.0)
    chans = [G]
    if add_h:
        hs = second_derivative(S, compat)
        hmin, hmax = h_extremes(hs, flt)
        _, q, f = h_scaled(hs, hmin, hmax)
        chans.append(np.where(np.isfinite(hs), f, F32(0)).astype(F32) if flt else q)
    nrm = P.normal_bytes(P.blur_gradient(S) if blur else S)
    if ring == "u16":
        chans = [U.quantize_u16(ch) for ch in chans]
    out = np.empty(F.shape[:3] + (nf + len(chans),), F.dtype)
    bits = np.uint32 if ring == "f32" else F.dtype
    out.view(bits)[..., :nf] = F.view(bits)
    for k, ch in enumerate(chans):
        out[..., nf + k] = ch
    return out, nrm


def downloaded(data, grad, normals=True):
    return M.downloaded(data, grad, normals)


# ---- volumes

# every axis one less than, equal to, and one to three more than a whole number of tiles, two tiles at least per axis; odd
# and even nx (a pad column of 8-byte voxels)
SHAPES = ((64, 16, 16), (63, 15, 15), (65, 17, 17), (66, 18, 18), (67, 19, 19))
MAIN = SHAPES[2]
TINY = (3, 3, 3)
NFS = {"u8": (1, 2), "u16": (1,), "f32": (1, 2)}     # with add_h; nf 3 (u8, f32) and u16 nf 2 take blur alone
FLAGS = tuple((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1))   # (add_h, blur, compat)


# dims -> the seed of its fields: the first under which no extreme of any case lies in the first tile (qualified case by
# case in tests/test_step_merge_h_cpu.py)
SEED = {(64, 16, 16): 1, (63, 15, 15): 11, (65, 17, 17): 0, (66, 18, 18): 0, (67, 19, 19): 13}


def field8(e, dims, seed):
    """field e as bytes: M.field8's smooth structure and noise without its flat block (whose edges would hold every extreme
    of H in the first tile), and a zero-gradient interior voxel at (1, 1, 1): its neighbours are equal in pairs"""
    nx, ny, nz = dims
    rng = np.random.default_rng(1000 * seed + 10 * e + 3)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = (np.sin(x * (.31 + .07 * e) + seed) * 55 + np.cos(y * (.23 + .05 * e) + z * (.47 - .06 * e) + e) * 50 + 128 +
         rng.normal(0, 5, x.shape))
    v = np.clip(v, 0, 255).astype(np.uint8)
    v[0, 1, 1], v[1, 0, 1], v[1, 1, 0] = v[2, 1, 1], v[1, 2, 1], v[1, 1, 2]
    return v


def fields(ring, nf, dims, seed=None):
    """[z][y][x][nf] of the ring's type; the seed is the one under which no extreme lies in the first tile (SEED)"""
    seed = SEED.get(tuple(dims), 0) if seed is None else seed
    return np.ascontiguousarray(np.stack([M.as_type(field8(e, dims, seed), ring) for e in range(nf)], -1))


def tile_of(zyx):
    return tuple(c // t for c, t in zip(zyx, TILE[::-1]))


def extremes_at(F, compat=1):
    """the voxels [z][y][x] at which the maximum magnitude, hmin and hmax of F are attained (the first of each)"""
    ring = RING_OF[np.ascontiguousarray(F).dtype]
    S = summed(np.ascontiguousarray(F).astype(F32))
    hs = second_derivative(S, compat)
    with np.errstate(**_IGNORE):
        mag = np.sqrt(S[..., 0] * S[..., 0] + S[..., 1] * S[..., 1] + S[..., 2] * S[..., 2])
    ok = np.zeros(hs.shape, bool)
    ok[1:-1, 1:-1, 1:-1] = True
    ok &= np.isfinite(hs) if ring != "u8" else ~np.isnan(hs)
    lo = np.where(ok, hs, np.inf)
    hi = np.where(ok, hs, -np.inf)
    return (np.unravel_index(np.argmax(np.where(np.isfinite(mag), mag, -1)), mag.shape), np.unravel_index(np.argmin(lo), lo.shape),
            np.unravel_index(np.argmax(hi), hi.shape)), hs


# more tiles than pass 1 has workgroups: 1 x 48 x 44 = 2112 tiles; the tiles from 2048 on are a workgroup's second turn, and
# they are those of the last layer of tiles (bz = 43, 43 * 48 = 2064 >= 2048): z >= 344
THIN = (5, 380, 350)
THIN_AT = (346, 200, 2)                # [z][y][x] of the planted maximum magnitude and, beside it, of both extremes of H
assert -(-380 // 8) == 48 and -(-350 // 8) == 44 and 48 * 44 > STATS_BLOCKS and (THIN_AT[0] // 8) * 48 >= STATS_BLOCKS


def thin_fields(ring, nf=1):
    return M.plant(M.fields(ring, nf, THIN), THIN_AT)


def source_step(F, add_h, seed=5):
    """a resident step that holds the fields F: (data [z][y][x][nf + 1 + add_h], normals) with last channels and normals that
    are NOT those of the fields"""
    nz, ny, nx, nf = F.shape
    rng = np.random.default_rng(seed)
    if F.dtype == np.float32:
        last = rng.random((nz, ny, nx, 1 + add_h)).astype(np.float32)
    else:
        last = rng.integers(0, 256, (nz, ny, nx, 1 + add_h)).astype(F.dtype) * (1 if F.dtype == np.uint8 else 257)
    return np.ascontiguousarray(np.concatenate([F, last], -1)), rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
