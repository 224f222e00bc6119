"""smk_blend_timesteps (include/smk.h, "Fractional time") restated in NumPy float32, from the header's contract and not
from the kernel: u = 1 - w once; per stored field r = (u * x) + (w * y), two products and one sum, each rounded to fp32; a
float field stores r, an integer field min((int)(r + 0.5f), top).  blend() works in the CALLER's layout and returns what a
host would have to upload so that the packed voxels are the ones the entry writes; wrong_*() are the three plausible
implementations the contract excludes, for tests/test_tblend_ref_cpu.py to tell apart.  The volumes and scenes the CPU
and the GPU tests share live here too.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from _scenes import make_scene, ragged_vgh, vgh_volume
from _u16_ref import decode_u16, q8, volume16

F = np.float32
WS_INT = (0.3, 0.7)                    # weights at which the wrong formulas show on integer voxels (test_tblend_ref_cpu)
WS_F32 = (0.3, 0.7, 1.0 / 3.0)


def _mix(x, y, w):
    w = F(w)
    u = F(1.0) - w
    with np.errstate(all="ignore"):
        return (u * np.asarray(x).astype(F)).astype(F) + (w * np.asarray(y).astype(F)).astype(F)


def _mix_int(x, y, w, top):
    r = _mix(x, y, w)
    return np.minimum((r + F(0.5)).astype(F).astype(np.int64), top)


def blend(data_a, grad_a, data_b, grad_b, w, dtype=None):
    """(data, grad) of the step (1 - w) a + w b; data [z][y][x][nelts] u8 / f32 / u16, grad [z][y][x][3] u8 or None"""
    dtype = np.dtype(dtype or data_a.dtype)
    assert data_a.dtype == dtype and data_b.dtype == dtype and data_a.shape == data_b.shape
    assert (grad_a is None) == (grad_b is None)
    if dtype == np.uint8:
        data = _mix_int(data_a, data_b, w, 255).astype(np.uint8)
    elif dtype == np.uint16:
        data = np.empty_like(data_a)
        for e in range(data_a.shape[-1]):
            if e < 2:
                data[..., e] = _mix_int(data_a[..., e], data_b[..., e], w, 65535)
            else:                      # the stored byte of the third channel is what is blended; q8(byte * 257) == byte
                data[..., e] = _mix_int(q8(data_a[..., e]), q8(data_b[..., e]), w, 255) * 257
    else:
        assert dtype == np.float32
        data = _mix(data_a, data_b, w)
    grad = None if grad_a is None else _mix_int(grad_a, grad_b, w, 255).astype(np.uint8)
    return np.ascontiguousarray(data), (None if grad is None else np.ascontiguousarray(grad))


# ---- what the contract excludes (x, y arrays of one field; integer fields with their top)

def _store(r, top):
    if top is None:
        return r.astype(F)
    return np.minimum((r.astype(F) + F(0.5)).astype(F).astype(np.int64), top)


def wrong_lerp(x, y, w, top=None):
    """x + w (y - x) in fp32"""
    x, y, w = np.asarray(x).astype(F), np.asarray(y).astype(F), F(w)
    return _store(x + (w * (y - x).astype(F)).astype(F), top)


def wrong_f64(x, y, w, top=None):
    """the blend in double, rounded once"""
    x, y, w = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64), np.float64(F(w))
    r = (1.0 - w) * x + w * y
    if top is None:
        return r.astype(F)
    return np.minimum((r + 0.5).astype(np.int64), top)


def wrong_fma(x, y, w, top=None):
    """fma(u, x, w * y): the first product unrounded (exact in double: 24 x 24 bits)"""
    w = F(w)
    u = F(1.0) - w
    x, y = np.asarray(x).astype(F), np.asarray(y).astype(F)
    r = np.float64(u) * x.astype(np.float64) + (w * y).astype(F).astype(np.float64)
    return _store(r.astype(F), top)


def right(x, y, w, top=None):
    return _mix(x, y, w) if top is None else _mix_int(x, y, w, top)


# ---- the volumes and scenes of the tests: 32^3 steps (seeds = time steps), 64^2 pixels x 64 planes

@functools.lru_cache(maxsize=None)
def step(dtype, seed, dims=None, nelts=3, normals=True):
    """(data, grad) of time step `seed`: dtype 'u8' | 'f32' | 'u16'; dims None = 32^3 of the reference generator's spheres"""
    if dtype == "u16":
        d, nrm = volume16(tuple(dims or (32, 32, 32)), seed)
        data = d
    else:
        v8, vf, nrm = ragged_vgh(tuple(dims), seed) if dims else vgh_volume(32, seed)
        data = v8 if dtype == "u8" else vf
    if nelts == 4:                     # a fourth channel that depends on the step
        extra = data[::-1, :, :, :1] if dtype != "f32" else (F(1.0) - data[..., 1:2]).astype(F)
        data = np.concatenate([data, extra], -1)
    data = np.ascontiguousarray(data[..., :nelts])
    data.setflags(write=False)
    return data, (nrm if normals else None)


@functools.lru_cache(maxsize=None)
def blended(dtype, sa, sb, w, dims=None, nelts=3, normals=True):
    a, b = step(dtype, sa, dims, nelts, normals), step(dtype, sb, dims, nelts, normals)
    data, grad = blend(a[0], a[1], b[0], b[1], w)
    data.setflags(write=False)
    return data, grad


def scene(data, grad, kind=None, pert=False, checker=False):
    """the config 3 scene (1-D table for one channel) over a volume; checker: u16 decoded, for the CPU checker's render()"""
    nz, ny, nx, ne = data.shape
    sc = make_scene(kind or ("cfg1" if ne == 1 else "cfg3"), n=32, size=64, steps=64, pose="diag", f32=True, shade=1, pert=pert)
    if checker and data.dtype == np.uint16:
        data = decode_u16(data)
    m = float(max(nx, ny, nz))
    sc.data, sc.grad, sc.dims, sc.nelts = data, grad, (nx, ny, nz), ne
    sc.fsize = tuple(F(v) for v in (nx / m, ny / m, nz / m))
    return sc
