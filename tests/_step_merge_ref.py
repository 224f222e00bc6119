"""Volumes and expected arrays of the step-merge tests (smk.h smk_merge_timestep, smk_upload_timestep_fields_device):
tests/test_gpu_step_merge.py.

The contract is the output of the recipe "Merged fields of a blend" (INTEGRATION.md 5): what the existing merge entries make
of a step's fields, uploaded.  Expected arrays therefore come from the restatements those entries are already held to:
O.merge_addg (the CPU checker, u8), _prep_f32_ref.merge_fields_f32 and _u16_ref.quantize_u16.  No GPU here;
tests/test_step_merge_cpu.py qualifies the volumes so that no GPU test can pass vacuously.

Volumes are [z][y][x][nf]; dims are (nx, ny, nz)."""
import numpy as np

import _prep_f32_ref as P
import _u16_ref as U

DIMS = ((37, 13, 11), (70, 21, 19))    # odd x: a pad column of 8-byte voxels; several tiles in y and z
SMALL = DIMS[0]
RINGS = ("u8", "u16", "f32")
NFS = {"u8": (1, 2, 3), "u16": (1, 2), "f32": (1, 2, 3)}      # a u16 voxel holds three channels
NP = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
CODE = {"u8": 0, "f32": 1, "u16": 2}   # smk_dtype
RING_OF = {np.dtype(np.uint8): "u8", np.dtype(np.uint16): "u16", np.dtype(np.float32): "f32"}
CASES = tuple((r, nf) for r in RINGS for nf in NFS[r])


def field8(e, dims, seed=0):
    """field e of a series' step `seed` as bytes: smooth structure in all three axes plus noise, and a flat block (zero
    gradient in every field)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(1000 * seed + 10 * e + 3)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    v = (np.sin(x * (.31 + .07 * e) + seed) * 55 + np.cos(y * (.23 + .05 * e) + z * (.47 - .06 * e) + e) * 50 + 128 +
         rng.normal(0, 5, x.shape))
    v = np.clip(v, 0, 255).astype(np.uint8)
    if nz > 8 and ny > 9 and nx > 11:
        v[2:7, 3:8, 4:10] = 77 + e
    return v


def as_type(v8, ring):
    """bytes as values of another type with the same structure: u16 spreads them over 16 bits, f32 over [0, 1]"""
    if ring == "u8":
        return v8
    if ring == "u16":
        return (v8.astype(np.uint16) * 257 + (v8.astype(np.uint16) % 7) * 5).astype(np.uint16)
    return (v8.astype(np.float32) / np.float32(255.0) + (v8 % 5).astype(np.float32) * np.float32(1e-3)).astype(np.float32)


def fields(ring, nf, dims, seed=0):
    """[z][y][x][nf] of the ring's type"""
    return np.ascontiguousarray(np.stack([as_type(field8(e, dims, seed), ring) for e in range(nf)], -1))


def noise(ring, nf, dims):
    """full-range noise: a wrong neighbour at a tile seam changes G and the normal"""
    nx, ny, nz = dims
    v = np.random.default_rng(nx * 10000 + ny * 100 + nz + nf).integers(0, 256, (nz, ny, nx, nf), dtype=np.uint8)
    return np.ascontiguousarray(np.stack([as_type(v[..., e], ring) for e in range(nf)], -1))


# ---- the tiles of the merge kernels (csrc/smk_step_merge.hip): MG_UX 16-byte units x MG_TY rows x MG_TZ slices

TILE = {"u8": (128, 4, 4), "u16": (128, 4, 4), "f32": (64, 4, 4)}      # in voxels (x, y, z)
MAX_BLOCKS = 2048                      # MG_MAX_BLOCKS: pass 1's grid is capped there and strides over the tiles


def tile_shapes(ring):
    """volumes at the tile's edges: a whole number of tiles, one voxel short, one and two past, in each axis; nx odd and even"""
    tx, ty, tz = TILE[ring]
    return ((tx, 2 * ty, 2 * tz), (tx - 1, 2 * ty - 1, 2 * tz - 1), (tx + 1, 2 * ty + 1, 2 * tz + 1), (tx + 2, 2 * ty + 2, 2 * tz + 2),
            (2 * tx, ty, tz), (2 * tx + 1, ty + 1, tz + 2), (tx // 2 + 1, ty - 1, tz + 1))


def plant(F, at):
    """F with the largest summed gradient planted at the interior voxel `at` = (z, y, x): the fields are compressed into the
    middle fifth of their range, then the two x neighbours of `at` take the range's ends in every field.  The magnitude at
    `at` is the whole range times nf; every other difference that a planted voxel enters is at most 0.6 of the range"""
    ring = RING_OF[F.dtype]
    z, y, x = at
    nz, ny, nx, nf = F.shape
    assert 1 <= z <= nz - 2 and 1 <= y <= ny - 2 and 1 <= x <= nx - 2
    if ring == "f32":
        G = (np.float32(0.4) + F * np.float32(0.2)).astype(np.float32)
        lo, hi = np.float32(0.0), np.float32(1.0)
    else:
        top = 255 if ring == "u8" else 65535
        G = (top * 2 // 5 + F.astype(np.int64) // 5).astype(F.dtype)
        lo, hi = 0, top
    G[z, y, x - 1, :] = lo
    G[z, y, x + 1, :] = hi
    return np.ascontiguousarray(G)


def planted_last(ring, nf, dims):
    """(fields, the voxel) of a maximum planted at the last interior voxel there is: in the last tile of the volume, or, where
    that holds border voxels only, in the one before it"""
    nx, ny, nz = dims
    at = (nz - 2, ny - 2, nx - 2)
    return plant(noise(ring, nf, dims), at), at


# more tiles than pass 1 has workgroups: 1 x 48 x 44 = 2112 tiles of either width; the tiles from 2048 on are a workgroup's
# second turn, and they are those of the last layer of tiles, bz = 43 (43 * 48 = 2064 >= 2048 > 42 * 48): z >= 172
THIN = (5, 190, 175)
THIN_AT = (173, 100, 2)                # [z][y][x]
assert (190 + 3) // 4 == 48 and (175 + 3) // 4 == 44 and 48 * 44 > MAX_BLOCKS and (THIN_AT[0] // 4) * 48 >= MAX_BLOCKS


def thin_fields(ring, nf=2):
    return plant(fields(ring, nf, THIN), THIN_AT)


# ---- the contract

def central_sum(Ff):
    """the summed gradient [z][y][x][3] of float fields [z][y][x][nf], as the contract states it: 0 on the border, fields
    ascending, one fp32 subtraction and one add per field and axis"""
    g = np.zeros(Ff.shape[:3] + (3,), np.float32)
    with np.errstate(all="ignore"):
        for e in range(Ff.shape[-1]):
            g = g + P.central_differences(np.ascontiguousarray(Ff[..., e]))
    return g


def magnitude(F):
    """|summed gradient| [z][y][x] in fp32 of fields of any type ((float)v of integers, unscaled)"""
    g = central_sum(np.ascontiguousarray(F).astype(np.float32))
    with np.errstate(all="ignore"):
        return np.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2])


def merge(O, F):
    """(data [z][y][x][nf + 1] of the fields' type, normals [z][y][x][3] u8) of the multi-field step of F in a ring of F's
    type: the header's table.  u8 is the CPU checker's mergeMV (undefined where the maximum is 0: not called then)"""
    F = np.ascontiguousarray(F)
    ring = RING_OF[F.dtype]
    nf = F.shape[-1]
    if ring == "u8":
        assert magnitude(F).max() > 0, "the checker divides by the maximum"
        return O.merge_addg(F)
    if ring == "f32":
        return P.merge_fields_f32(F)
    out, nrm = P.merge_fields_f32(F.astype(np.float32))
    return np.ascontiguousarray(np.concatenate([F, U.quantize_u16(out[..., nf])[..., None]], -1)), nrm


def g_without(F, at):
    """the float G [z][y][x] of F with voxel `at` left out of the maximum: what a pass 1 that dropped its tile would give"""
    mag = magnitude(F).astype(np.float32)
    rest = mag.copy()
    rest[at] = 0
    with np.errstate(all="ignore"):
        return (mag / rest.max()).astype(np.float32), (mag / mag.max()).astype(np.float32)


def downloaded(data, grad, normals=True):
    """what smk_download_timestep returns of an uploaded (data, grad): a u16 third channel comes back as 257 * its stored
    byte; a context without normals gives (128, 128, 128)"""
    data = np.ascontiguousarray(data)
    if data.dtype == np.uint16 and data.shape[-1] > 2:
        data = data.copy()
        data[..., 2] = 257 * ((data[..., 2].astype(np.int64) * 255 + 32767) // 65535)
    grad = np.ascontiguousarray(grad) if normals else np.full(data.shape[:3] + (3,), 128, np.uint8)
    return data, grad


def source_step(F, seed=5):
    """a resident step that holds the fields F: (data [z][y][x][nf + 1], normals) with a last channel and normals that are
    NOT those of the fields -- the merge must replace both"""
    nz, ny, nx, nf = F.shape
    rng = np.random.default_rng(seed)
    if F.dtype == np.float32:
        last = rng.random((nz, ny, nx, 1)).astype(np.float32)
    else:
        last = rng.integers(0, 256, (nz, ny, nx, 1)).astype(F.dtype) * (1 if F.dtype == np.uint8 else 257)
    return np.ascontiguousarray(np.concatenate([F, last], -1)), rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
