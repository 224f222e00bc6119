"""Volumes and expected arrays of the step-derivation tests (smk.h smk_derive_timestep, smk_upload_timestep_scalar_device).

The contract is the output of the recipe "Derivatives of a blend" (INTEGRATION.md 5): what the existing preparation entries
make of a step's scalar, uploaded.  Expected arrays therefore come from the restatements those entries are already held to:
O.make_vgh and O.normals_vgh (the CPU checker), _prep_f32_ref.normals_f32 and _u16_ref.quantize_u16.  No GPU here;
tests/test_step_derive_cpu.py qualifies the volumes so that no GPU test can pass vacuously.

Volumes are [z][y][x]; dims are (nx, ny, nz)."""
import numpy as np

import _prep_f32_ref as P
import _tblend_ref as T
import _u16_ref as U

DIMS = ((70, 21, 19), (37, 13, 11))    # odd x: a pad column of 8-byte voxels; ragged tiles; the larger has two tiles per axis
SMALL = DIMS[1]
W = 0.37
CASES = ((1, 0), (0, 1))               # (compat, blur)
RINGS = ("u8", "u16", "f32")
NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
CODE = {"u8": 0, "f32": 1, "u16": 2}   # smk_dtype


def scalar(s, dims):
    """the u8 scalar of step s: test_derivatives_of_a_blend_on_the_device's formula, and a flat block (zero gradients)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(24 + s)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = np.clip(np.sin(x * (.3 + .1 * s)) * 60 + np.cos(y * .2 + z * .5 + s) * 50 + 128 + rng.normal(0, 4, x.shape), 0, 255)
    v = v.astype(np.uint8)
    v[2:7, 3:8, 4:10] = 77 + s
    return v


def as_type(v8, kind):
    """a u8 scalar as a scalar of another type with the same structure: u16 spreads it over 16 bits, f32 over [0, 1]"""
    if kind == "u8":
        return v8
    if kind == "u16":
        return (v8.astype(np.uint16) * 257 + (v8.astype(np.uint16) % 7) * 5).astype(np.uint16)
    return (v8.astype(np.float32) / np.float32(255.0) + (v8 % 5).astype(np.float32) * np.float32(1e-3)).astype(np.float32)


def derive(O, s, ring, compat=1, blur=0):
    """(data [z][y][x][3] of the ring's type, normals [z][y][x][3] u8) of the VGH step of the scalar s [z][y][x]
    (u8, u16 or f32) in a ring of type `ring`: the header's table.  A u16 scalar takes the float path on the same values."""
    s = np.ascontiguousarray(s)
    v8, vf = O.make_vgh(s if s.dtype == np.uint8 else s.astype(np.float32), compat=bool(compat), f32=True)
    if ring == "u8":
        return v8, O.normals_vgh(v8, blur=bool(blur))
    nrm = P.normals_f32(vf, blur=bool(blur))
    return (vf if ring == "f32" else U.quantize_u16(vf)), nrm


def series_step(O, v8, ring):
    """a step of the series the host prepared from the u8 scalar v8: (data, normals), compat 1, plain normals"""
    return derive(O, v8, ring, 1, 0)


def blended(O, dims, ring, w=W):
    """(step 0, step 1, their blend) of the series of `ring`, each (data, normals)"""
    a, b = (series_step(O, scalar(s, dims), ring) for s in (0, 1))
    return a, b, T.blend(a[0], a[1], b[0], b[1], w)


def downloaded(data, grad):
    """what smk_download_timestep returns of an uploaded (data, grad): a u16 third channel comes back as 257 * its stored byte"""
    data = np.ascontiguousarray(data)
    if data.dtype == np.uint16:
        data = data.copy()
        data[..., 2] = 257 * ((data[..., 2].astype(np.int64) * 255 + 32767) // 65535)
    return data, np.ascontiguousarray(grad)
