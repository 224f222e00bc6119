"""Volumes and expected arrays of the step-derivation tests (smk.h smk_derive_timestep, smk_upload_timestep_scalar_device):
tests/test_gpu_step_derive.py, tests/test_gpu_step_derive_shapes.py and the float and second-grid-turn cases of
tests/test_gpu_prep.py.

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


# ---- float scalars away from [0, 1] (tests/test_gpu_prep.py, tests/test_gpu_step_derive_shapes.py)

SCALARS = ("u8", "u16", "f32", "signed", "above", "below")     # what typed() makes of a u8 scalar
KIND = {"u8": "u8", "u16": "u16", "f32": "f32", "signed": "f32", "above": "f32", "below": "f32"}
ALL_CASES = CASES + ((0, 0), (1, 1))   # (compat, blur): each flag with each value of the other


def small_scalar(dims):
    """a u8 scalar of noise for a volume too small for scalar()'s flat block: the six neighbours of the interior voxel
    (1, 1, 1) are equal, so that its gradient is zero and its H is NaN"""
    nx, ny, nz = dims
    v = np.random.default_rng(nx * 100 + ny * 10 + nz).integers(0, 256, (nz, ny, nx), dtype=np.uint8)
    for z, y, x in ((0, 1, 1), (2, 1, 1), (1, 0, 1), (1, 2, 1), (1, 1, 0), (1, 1, 2)):
        v[z, y, x] = 77
    return v


def minus_zero_at(shape):
    """the voxel [z][y][x] that typed(.., "signed") sets to -0.0: interior, and not a neighbour of a zero-gradient voxel"""
    nz, ny, nx = shape
    return nz // 2, ny // 2, nx // 2


def typed(v8, name):
    """the u8 scalar v8 as the scalar `name` of SCALARS, with the same structure (a flat block stays flat):
    "signed" is the f32 scalar times 15.5 minus 3.5, about -3.5 .. 12.1, with one -0.0 voxel: the negative branch of the
              ordered-int map decides dmin, and 0 lies inside the range;
    "above"  is (signed + 4) * 3e8, wholly above the reference's seed 1e8 of the running minimum: dmin is the SEED;
    "below"  is its negation, wholly below the seed -1e8 of the running maximum: dmax is the seed."""
    if name in ("u8", "u16", "f32"):
        return as_type(v8, name)
    s = (as_type(v8, "f32") * np.float32(15.5) - np.float32(3.5)).astype(np.float32)
    s[minus_zero_at(s.shape)] = np.float32(-0.0)
    if name == "signed":
        return s
    s = ((s + np.float32(4.0)) * np.float32(3e8)).astype(np.float32)
    return s if name == "above" else (-s).astype(np.float32)


# ---- tile-edge shapes: the derive kernels work on tiles of 32 x 8 x 8 voxels with a 2-voxel apron

TILE = (32, 8, 8)
# every nx of 31..34 and 63..65, every ny of 7..10, 16, 17, every nz of 8, 9, 10, 17; two shapes are whole tiles on every axis
TILE_SHAPES = ((32, 8, 8), (64, 16, 8), (31, 7, 9), (33, 9, 10), (34, 10, 17), (63, 17, 8), (65, 8, 9), (31, 16, 10),
               (34, 9, 9), (65, 10, 10))
TILE_CASES = ((1, 0), (0, 1))          # blur off and on


def noise(dims):
    """a u8 scalar of full-range noise: a wrong neighbour at a tile seam changes bytes"""
    nx, ny, nz = dims
    return np.random.default_rng(nx * 10000 + ny * 100 + nz).integers(0, 256, (nz, ny, nx), dtype=np.uint8)


def last_tile(dims):
    """the slices [z][y][x] of the voxels of the last tile along each axis"""
    return tuple(slice(t * ((n - 1) // t), n) for n, t in zip(dims[::-1], TILE[::-1]))


# ---- more tiles than the stats grid

THIN = (5, 377, 361)                   # 1 x 48 x 46 tiles
STATS_BLOCKS = 2048                    # DV_STATS_BLOCKS (csrc/smk_step_derive.hip): the stats pass's grid is capped there
SECOND_TURN_Z = 344                    # every tile with bz >= 43 has an index >= 43 * 48 = 2064: a workgroup's second tile
assert 48 * 46 > STATS_BLOCKS and (SECOND_TURN_Z // TILE[2]) * 48 >= STATS_BLOCKS
PLANT = ((352, 100, 2), (352, 101, 2))  # [z][y][x] of the only 0 and the only 255: interior, side by side, z >= 350


def thin_scalar():
    """the u8 scalar of THIN: scalar()'s field compressed into 40..215, and the only 0 and the only 255 planted side by side
    -- the extremes of the data and, next to them, of G and H -- where only a second turn of the stats loop sees them"""
    v = scalar(0, THIN).astype(np.int32)
    v = (40 + v * 175 // 255).astype(np.uint8)
    v[PLANT[0]], v[PLANT[1]] = 0, 255
    return v


# ---- more voxels than the grids of the byte preparation entries

BIG = (129, 128, 128)
VGH_THREADS = 4096 * 256               # smk_make_vgh_device's grid cap (csrc/smk_prep.hip)
NRM_THREADS = 8192 * 256               # smk_normals_vgh_device's
assert 129 * 128 * 128 > NRM_THREADS and 129 * 128 * 128 > 2 * VGH_THREADS
BIG_MIN, BIG_MAX = (70, 64, 64), (126, 126, 127)      # [z][y][x] of the interior extremes


def big_scalar():
    """the u8 scalar of BIG: a field in 40..215; the interior minimum 5 and maximum 250 where only a second grid turn of
    smk_make_vgh_device reads them (linear index > 1 048 576), the maximum in the last interior voxel there is.  No
    INTERIOR voxel has a linear index beyond 2 097 152 -- those 16 384 voxels all lie in the last slice, which is border --
    so the scalar's global 0 and 255 are put there: a third turn that took them for data, or a second turn of the normals
    kernel that left the blurred border out, shows."""
    nx, ny, nz = BIG
    rng = np.random.default_rng(129)
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float32), np.arange(ny, dtype=np.float32), np.arange(nx, dtype=np.float32),
                          indexing="ij", sparse=True)
    v = np.sin(x * .3) * 60 + np.cos(y * .2 + z * .5) * 50 + 128 + rng.normal(0, 4, (nz, ny, nx)).astype(np.float32)
    v = (40 + np.clip(v, 0, 255).astype(np.int32) * 175 // 255).astype(np.uint8)
    v[2:7, 3:8, 4:10] = 77
    v[BIG_MIN], v[BIG_MAX] = 5, 250
    v[127, 100, 50], v[127, 101, 50] = 0, 255
    return v


def linear(zyx, dims):
    return (zyx[0] * dims[1] + zyx[1]) * dims[0] + zyx[2]


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
