"""smk_hist2d_step[_device], smk_hist2d_finish and smk_probe_step (include/smk.h, "the histogram and the probe of a RESIDENT
time step") restated in NumPy from the header's contract, not from the kernels, on the CALLER's arrays [z][y][x][nelts]:
  bins     u8 the byte; f32 t = v * 255.0f in fp32, NaN or t < 0 -> 0, t >= 255 -> 255, else (int)t; u16 v // 257;
  counts   counts[b1][b0] over the voxels of a box [g0, g1) (x, y, z), each once;
  finish   min(count, 2^24) as float32, h = (float)log(count), byte = (uchar)(h / max * 255) in fp32, 0 for an empty bin and
           when no bin holds more than one voxel;
  probe    the stored values of a cell's eight corners, corner i * 4 + j * 2 + k = voxel (x + k, y + j, z + i).
The volumes and shard cases the CPU and the GPU tests share live here too.  TEST INFRASTRUCTURE ONLY."""
import functools
import math

import numpy as np

F = np.float32
DIMS = (41, 37, 45)                    # (nx, ny, nz): all odd, 68 265 voxels -- more than one flush chunk of 61 440
CHUNK = 61440
SHARD_CASES = [(n, h) for n in (2, 4, 8) for h in (1, 3)]
U16_EDGES = ((0, 0), (256, 0), (257, 1), (513, 1), (65534, 254), (65535, 255))


def bin_u16(v):
    return (np.asarray(v).astype(np.int64) // 257).astype(np.uint8)


def bin_f32(v):
    with np.errstate(all="ignore"):
        t = (np.asarray(v, F) * F(255.0)).astype(F)
        mid = (t >= F(0)) & (t < F(255))
        b = np.where(mid, t, F(0)).astype(np.int32)        # (NaN compares false both ways: bin 0)
    b[t >= F(255)] = 255
    return b.astype(np.uint8)


def bins(data):
    """(b0, b1) of a volume with at least two channels, by its dtype"""
    assert data.shape[-1] >= 2
    f = {np.dtype(np.uint8): lambda v: np.asarray(v), np.dtype(np.float32): bin_f32, np.dtype(np.uint16): bin_u16}[data.dtype]
    return f(data[..., 0]), f(data[..., 1])


def counts(data, g0=None, g1=None):
    """[256][256] uint32, counts[b1][b0], of the voxels of the box [g0, g1) (default: the whole volume)"""
    if g0 is not None:
        data = data[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]]
    b0, b1 = bins(data)
    key = b1.astype(np.int64).ravel() * 256 + b0.ravel()
    return np.bincount(key, minlength=65536).astype(np.uint32).reshape(256, 256)


def finish(c):
    """the log-scaled bytes of 65536 counts"""
    ih = np.minimum(np.asarray(c, np.int64).ravel(), 1 << 24)
    u, inv = np.unique(ih, return_inverse=True)             # (libm's log, as the library calls it)
    lg = np.array([math.log(float(F(x))) if x > 0 else -np.inf for x in u], F)[inv.ravel()]
    mx = max(F(0), lg.max())
    hist = np.zeros(65536, np.uint8)
    if mx > 0:
        ok = np.isfinite(lg)
        hist[ok] = ((lg[ok] / F(mx)).astype(F) * F(255)).astype(F).astype(np.int32).astype(np.uint8)
    return hist.reshape(256, 256)


def q8(c):
    """the stored 8-bit value of a u16 voxel's third channel (smk.h SMK_U16)"""
    return (np.asarray(c).astype(np.int64) * 255 + 32767) // 65535


def probe(data, grad, cells, box=None):
    """(raw [n][8][4] float32, nrm [n][8][3] uint8, ok [n] bool) of smk_probe_step on a context that stores box = (origin,
    size) of the volume (default: all of it; a pad column past the volume does not count)"""
    nz, ny, nx, ne = data.shape
    N = (nx, ny, nz)
    o, d = box or ((0, 0, 0), N)
    lo = [max(o[a], 0) for a in range(3)]
    hi = [min(o[a] + d[a], N[a]) for a in range(3)]
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    n = len(cells)
    raw, nrm, ok = np.zeros((n, 8, 4), F), np.zeros((n, 8, 3), np.uint8), np.zeros(n, bool)
    for m, c in enumerate(cells):
        ok[m] = all(lo[a] <= c[a] and c[a] + 1 <= hi[a] - 1 for a in range(3))
        if not ok[m]:
            continue
        for i in range(2):
            for j in range(2):
                for k in range(2):
                    v = data[c[2] + i, c[1] + j, c[0] + k]
                    s = raw[m, i * 4 + j * 2 + k]
                    if data.dtype == np.uint16:
                        s[:min(ne, 2)] = v[:2]
                        if ne > 2:
                            s[2] = q8(v[2])
                    else:
                        s[:ne] = v
                    nrm[m, i * 4 + j * 2 + k] = grad[c[2] + i, c[1] + j, c[0] + k] if grad is not None else 128
    return raw, nrm, ok


# ---- the volumes of the tests

@functools.lru_cache(maxsize=None)
def volume(dtype, nelts, seed=1, dims=DIMS):
    """(data [z][y][x][nelts], grad [z][y][x][3]) of seeded random voxels: 'u8' | 'f32' (values in [-0.1, 1.1)) | 'u16'; the
    first three z slices are one value (whole waves in one bin), the next three take few values (contended bins)"""
    nx, ny, nz = dims
    rng = np.random.default_rng(1000 * seed + {"u8": 1, "f32": 2, "u16": 3}[dtype])
    shape = (nz, ny, nx, nelts)
    if dtype == "u8":
        data = rng.integers(0, 256, shape, dtype=np.uint8)
        data[:3], data[3:6] = 7 + seed, data[3:6] & 0xC0
    elif dtype == "u16":
        data = rng.integers(0, 65536, shape, dtype=np.uint16)
        data[:3], data[3:6] = 700 + seed, data[3:6] & 0xC000
    else:
        data = (rng.random(shape) * 1.2 - 0.1).astype(F)
        data[:3], data[3:6] = F(0.031) * seed, (np.round(data[3:6] * 4) / 4).astype(F)
    grad = rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
    data.setflags(write=False)
    grad.setflags(write=False)
    return data, grad


def shard_rows(dims, rank, nranks, halo, u8):
    """(run length g1x - g0x, first voxel's offset g0x - Ox in the stored box) of a shard's rows"""
    from _layouts import stored_box
    from simian_spacemonkey_amd import sortlast
    g0, g1 = sortlast.shard_region(dims, rank, nranks)
    o, _ = stored_box(dims, rank, nranks, u8, halo)
    return g1[0] - g0[0], g0[0] - o[0]
