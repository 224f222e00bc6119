"""smk_download_timestep[_device] and smk_get_timestep_box (include/smk.h, "a resident time step read back") restated in
NumPy from the header's contract and DESIGN.md section 3, not from the kernels:
  pack      the four packed layouts of a voxel, as 32-bit words:
              u8   {c0 | c1 << 8 | c2 << 16 | c3 << 24,  n0 | n1 << 8 | n2 << 16}
              u16  {c0 | c1 << 16,  n0 | n1 << 8 | n2 << 16 | q8(c2) << 24},  q8(c) = (255 c + 32767) // 65535
              f32  {c0, c1, c2, normal word}            (up to three channels)
              f32  {c0, c1, c2, c3} + a separate normal word   (four channels)
            a missing channel is 0, a missing normal (128, 128, 128);
  unpack    the download rule on those words: the stored fields, nothing rescaled; u16 channel 2 comes back as 257 * q;
  region    the box of shard `rank` of `nranks`: bit 0 of the rank halves x at N // 2, bit 1 y, bit 2 z.
The volumes the CPU and the GPU tests share live here too: per-voxel random noise, so that one misplaced voxel shows; f32
volumes draw raw 32-bit patterns (NaNs with payloads, infinities, -0, denormals) for a share of their voxels and are compared
as uint32.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

NP = {"u8": np.uint8, "f32": np.float32, "u16": np.uint16}
CODE = {"u8": 0, "f32": 1, "u16": 2}                     # smk_dtype
DMODE = {1: "V1", 2: "V1G", 3: "VGH", 4: "V2GH"}
SMALL = (9, 7, 5)                      # all odd: 8-byte rows carry the pad voxel, a 3-byte row of 9 voxels is 27 bytes
LONG = (1100, 3, 3)                    # a row of more f32 voxels than the 1024 units a workgroup takes at a time
LONGER = (2101, 3, 2)                  # ... and of more 8-byte voxel pairs: 1051 units, an odd run
LAYOUTS = [(d, n) for d in ("u8", "f32") for n in (1, 2, 3, 4)] + [("u16", n) for n in (1, 2, 3)]
SHARD_CASES = [(n, h) for n in (2, 4, 8) for h in (1, 3)]
GUARD = 64


def q8(c):
    return (np.asarray(c).astype(np.int64) * 255 + 32767) // 65535


def bits(a):
    """an array for exact comparison: floats as their 32-bit patterns"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def pack(data, grad=None):
    """(words [z][y][x][2 or 4] uint32, separate normal words [z][y][x] uint32 or None) of a volume [z][y][x][nelts]"""
    data = np.ascontiguousarray(data)
    ne = data.shape[-1]
    if grad is None:
        nw = np.full(data.shape[:3], 0x00808080, np.uint32)
    else:
        g = np.asarray(grad).astype(np.uint32)
        nw = g[..., 0] | g[..., 1] << 8 | g[..., 2] << 16
    if data.dtype == np.uint8:
        w0 = np.zeros(data.shape[:3], np.uint32)
        for e in range(ne):
            w0 |= data[..., e].astype(np.uint32) << (8 * e)
        return np.stack([w0, nw], -1), None
    if data.dtype == np.uint16:
        assert ne <= 3
        w0 = data[..., 0].astype(np.uint32)
        if ne > 1:
            w0 = w0 | data[..., 1].astype(np.uint32) << 16
        w1 = nw | (q8(data[..., 2]).astype(np.uint32) << 24 if ne > 2 else np.uint32(0))
        return np.stack([w0, w1], -1), None
    assert data.dtype == np.float32
    w = np.zeros(data.shape[:3] + (4,), np.uint32)
    w[..., :ne] = data.view(np.uint32)
    if ne <= 3:
        w[..., 3] = nw
        return w, None
    return w, (nw if grad is not None else None)


def unpack(words, sep, dtype, nelts):
    """(data [z][y][x][nelts], grad [z][y][x][3] uint8): what a download returns of packed voxels"""
    words = np.asarray(words, np.uint32)
    shape = words.shape[:3]
    if dtype == "u8":
        data = np.stack([(words[..., 0] >> (8 * e)) & 255 for e in range(nelts)], -1).astype(np.uint8)
        nw = words[..., 1]
    elif dtype == "u16":
        ch = [words[..., 0] & 65535, words[..., 0] >> 16, 257 * (words[..., 1] >> 24)]
        data = np.stack(ch[:nelts], -1).astype(np.uint16)
        nw = words[..., 1]
    else:
        data = np.ascontiguousarray(words[..., :nelts]).view(np.float32)
        nw = words[..., 3] if nelts <= 3 else (sep if sep is not None else np.full(shape, 0x00808080, np.uint32))
    grad = np.stack([(nw >> (8 * a)) & 255 for a in range(3)], -1).astype(np.uint8)
    return np.ascontiguousarray(data), grad


def expected(data, grad=None):
    """(data, grad) a download returns of a step uploaded from (data, grad): the arrays themselves, but a u16 third channel as
    257 * q8 of it and missing normals as 128s"""
    data = np.ascontiguousarray(data)
    if data.dtype == np.uint16 and data.shape[-1] > 2:
        data = data.copy()
        data[..., 2] = 257 * q8(data[..., 2])
    if grad is None:
        grad = np.full(data.shape[:3] + (3,), 128, np.uint8)
    return data, np.ascontiguousarray(grad)


def region(dims, rank, nranks):
    """(g0, g1) of a shard (x, y, z)"""
    g0, g1 = [0, 0, 0], list(dims)
    bit, n = 0, nranks
    while n > 1:
        a, half = bit % 3, dims[bit % 3] // 2
        if (rank >> bit) & 1:
            g0[a] = max(g0[a], half)
        else:
            g1[a] = min(g1[a], half)
        n >>= 1
        bit += 1
    return tuple(g0), tuple(g1)


def cut(a, g0, g1):
    return np.ascontiguousarray(a[g0[2]:g1[2], g0[1]:g1[1], g0[0]:g1[0]])


SPECIALS = np.array([0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7fa5a5a5, 0x7f800000, 0xff800000, 0x80000000,
                     0x00000001, 0x807fffff, 0x00800000, 0x7f7fffff, 0xff7fffff], np.uint32)


@functools.lru_cache(maxsize=None)
def volume(dtype, nelts, dims=SMALL, seed=1, specials=True):
    """(data [z][y][x][nelts], grad [z][y][x][3]) of seeded per-voxel noise; f32 with specials: about one value in four is a
    raw 32-bit pattern -- half of them from SPECIALS, half any 32 bits"""
    nx, ny, nz = dims
    rng = np.random.default_rng(7000 * seed + 10 * CODE[dtype] + nelts)
    shape = (nz, ny, nx, nelts)
    if dtype == "u8":
        data = rng.integers(0, 256, shape, dtype=np.uint8)
    elif dtype == "u16":
        data = rng.integers(0, 65536, shape, dtype=np.uint16)
    else:
        w = (rng.random(shape) * 1.2 - 0.1).astype(np.float32).view(np.uint32)
        if specials:
            pick = rng.random(shape)
            w = np.where(pick < 0.125, SPECIALS[rng.integers(0, len(SPECIALS), shape)], w)
            w = np.where((pick >= 0.125) & (pick < 0.25), rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32), w)
        data = np.ascontiguousarray(w.astype(np.uint32)).view(np.float32)
    grad = rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8)
    data.setflags(write=False)
    grad.setflags(write=False)
    return data, grad
