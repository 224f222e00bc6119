"""Device memory and streams of the GPU tests.

THE RULE.  torch fills a new tensor with a kernel on its current stream, the null stream, and returns before that kernel has
run.  A context's own stream is made with hipStreamNonBlocking (smk_create), and a stream a test creates with
torch.cuda.Stream() is non-blocking too: neither waits for the null stream.  So a buffer that the library will write -- or
read -- must be complete before its address is handed over, or the fill lands on top of what the library wrote.  Every such
buffer is made by out_buffer() below or by something built on it (Guarded, words_buf, layer_buffer), which fill and THEN
synchronise, and an array goes to the device through dev_tensor() or dev_ptr(), which return when it is there; no test orders
a fill by hand.  A torch.cuda.synchronize() that is left in a test says what it orders.  These constructors wait for the WHOLE
device: a test whose point is that no host wait stands between two calls makes its buffers before the first of them.

torch is imported inside the functions: collecting the suite on a machine without a GPU does not load it."""
import ctypes

import numpy as np

import _step_read_ref as D


def out_buffer(shape, dtype, fill=0):
    """a device tensor of `shape` (an int: so many elements) and NumPy type `dtype`, every element `fill`, that the library may
    write at once: the fill runs on torch's null stream, which nothing orders against a context's non-blocking stream, so
    the device is synchronised before the tensor is returned"""
    import torch
    t = torch.full(shape if isinstance(shape, tuple) else (int(shape),), fill, dtype=getattr(torch, np.dtype(dtype).name), device="cuda")
    torch.cuda.synchronize()
    return t


class Guarded:
    """nbytes of device memory between guard bytes; `shift` more bytes in front move the buffer off the allocation's
    alignment (a multiple of the element size)"""

    def __init__(self, nbytes, shift=0):
        self.n, self.off = int(nbytes), D.GUARD + shift
        self.t = out_buffer(self.off + self.n + D.GUARD, np.uint8, 0xA5)
        self.ptr = self.t.data_ptr() + self.off

    def take(self, dtype, shape, what=""):
        h = self.t.cpu().numpy()
        assert (h[:self.off] == 0xA5).all(), "%s: bytes in front of the buffer were written" % what
        assert (h[self.off + self.n:] == 0xA5).all(), "%s: bytes behind the buffer were written" % what
        return h[self.off:self.off + self.n].copy().view(dtype).reshape(shape)


def words_buf(n=1):
    """n rows of the eight words a stencil producer's export writes, every word 0x5a5a5a5a"""
    return out_buffer((n, 8), np.int32, 0x5a5a5a5a)


def dev_tensor(a):
    """the array's bytes in device memory (a torch tensor that owns them); the copy from pageable host memory has ended when
    .cuda() returns"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def dev_ptr(a, shift=0):
    """(device address, the torch tensor that owns it) of the array's bytes, `shift` bytes behind the allocation's start"""
    import torch
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros(b.size + shift, dtype=torch.uint8, device="cuda")
    t[shift:] = torch.from_numpy(b.copy()).cuda()
    torch.cuda.synchronize()                                # the device copy into t runs on the null stream
    return t.data_ptr() + shift, t


def field_ptrs(F, shift=0):
    """(device addresses, owners) of the fields of F as separate dense arrays, as a simulation holds them"""
    ptrs, keep = [], []
    for e in range(F.shape[-1]):
        p, k = dev_ptr(np.ascontiguousarray(F[..., e]), shift)
        ptrs.append(p)
        keep.append(k)
    return ptrs, keep


def stream_arg(s):
    return ctypes.c_void_p(s.cuda_stream)


def busy(s, work):
    """a few milliseconds of work on stream s, so that what is enqueued behind it has not started when the next call is made"""
    import torch
    with torch.cuda.stream(s):
        for _ in range(24):
            work.add_(1)


# ---- the layers of all ranks, and their composite

def layer_buffer(rs, sc):
    """[P][W * H][4] floats of zeros for the layers of the ranks rs"""
    return out_buffer((len(rs), sc.width * sc.height, 4), np.float32)


def enqueue_layers(rs, layers, stream=None):
    for r, R in enumerate(rs):
        R.render_device(layers[r].data_ptr(), None, stream)


def fetch_layers(layers, sc):
    import torch
    torch.cuda.synchronize()                                # the frames ran on the contexts' streams, or the caller's: read-back
    return layers.cpu().numpy().reshape(layers.shape[0], sc.height, sc.width, 4)


def layers_of(rs, sc, stream=None):
    """every rank's layer of the scene, [P][H][W][4]"""
    layers = layer_buffer(rs, sc)
    enqueue_layers(rs, layers, stream)
    return fetch_layers(layers, sc)


def merged(rs, sc):
    """every rank's layer, composited in the ranks' visibility order on rank 0: (layers [P][H][W][4], frame [H][W][4])"""
    import torch
    npix = sc.width * sc.height
    layers = layer_buffer(rs, sc)
    out = out_buffer((npix, 4), np.float32)
    enqueue_layers(rs, layers)
    torch.cuda.synchronize()                                # rank 0's stream composites what every rank's stream rendered
    rs[0].composite_over_device(layers.data_ptr(), len(rs), rs[0].shard_order(len(rs)), npix, out.data_ptr(), None)
    return fetch_layers(layers, sc), out.cpu().numpy().reshape(sc.height, sc.width, 4)
