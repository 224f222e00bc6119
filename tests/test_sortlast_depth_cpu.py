"""First-hit depth through the torch.distributed sort-last path (simian-spacemonkey_amd/sortlast.py) on CPU: two gloo ranks
exchange 1/P tiles of their RGBA layer AND of their depth plane, composite the RGBA in order, merge the depth by minimum,
and gather both on rank 0.  The merged depth must be the minimum of the two ranks' planes (+inf where neither has a
sample), the RGBA the ordered over, and the tiles must reassemble in pixel order (the GPU path: tests/test_gpu_sortlast_depth.py)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cpu_over(layers, order):
    acc = torch.zeros_like(layers[0])
    for l in order:
        acc = acc + (1.0 - acc[:, 3:4]) * layers[l]
    return acc


def rank_layer(rank, npix):
    """a rank's layer: premultiplied RGBA and a depth plane, +inf (no sample) where its alpha is 0; pixel p's depth
    encodes p, so a tile delivered to the wrong place shows"""
    g = np.random.default_rng(1234 + rank)
    a = g.uniform(0.0, 1.0, npix).astype(np.float32)
    a[g.uniform(size=npix) < 0.35] = 0.0
    rgba = np.concatenate([g.uniform(0.0, 1.0, (npix, 3)).astype(np.float32) * a[:, None], a[:, None]], 1)
    depth = (np.arange(npix, dtype=np.float32) * 0.01 + g.uniform(1.0, 2.0, npix).astype(np.float32)).astype(np.float32)
    depth[a == 0] = np.inf
    return rgba, depth


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, npix, order, q):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import load_package
    load_package()
    from simian_spacemonkey_amd import sortlast
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        tp = sortlast.tile_pixels(npix, world)
        rgba, depth = rank_layer(rank, npix)
        part = torch.zeros((tp * world, 4))
        part[:npix] = torch.from_numpy(rgba)
        dpart = torch.full((tp * world,), float("inf"))
        dpart[:npix] = torch.from_numpy(depth)
        tile, dtile = sortlast.exchange_and_composite(part, order, cpu_over, depth=dpart)
        assert tile.shape == (tp, 4) and dtile.shape == (tp,)
        full, dfull = sortlast.gather_frame(tile, 0, depth=dtile)
        # the same with the caller's buffers (what Pipeline passes)
        into = torch.empty((world, tp, 4)) if rank == 0 else None
        dinto = torch.empty((world, tp)) if rank == 0 else None
        tile2, dtile2 = sortlast.exchange_and_composite(part, order, cpu_over, recv=torch.empty_like(part), depth=dpart,
                                                         recv_depth=torch.empty_like(dpart))
        full2, dfull2 = sortlast.gather_frame(tile2, 0, into=into, depth=dtile2, depth_into=dinto)
        if rank == 0:
            q.put((full[:npix].numpy().copy(), dfull[:npix].numpy().copy(), full2[:npix].numpy().copy(), dfull2[:npix].numpy().copy()))
        else:
            assert full is None and dfull is None
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("npix,order", [(40 * 30, [0, 1]), (37, [1, 0])])
def test_two_rank_depth_merges_by_minimum(npix, order):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, npix, order, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=120)
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    layers = [rank_layer(r, npix) for r in range(world)]
    want_d = np.minimum(layers[0][1], layers[1][1])
    acc = np.zeros((npix, 4), np.float32)
    for l in order:
        acc = acc + (1.0 - acc[:, 3:4]) * layers[l][0]
    assert np.isfinite(want_d).mean() > 0.3 and np.isinf(want_d).mean() > 0.05, "vacuous layers"
    for full, dfull in (got[:2], got[2:]):
        assert np.array_equal(dfull, want_d)
        assert np.abs(full - acc).max() <= 1e-6
