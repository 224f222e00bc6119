"""Cost of first-hit depth in the sort-last exchange (smk_exchange_*_depth): P = 2 / 4 / 8 shard contexts of
ONE process on one GPU (the in-process transport: tiles move by device-to-device copies), each renders its shard of a
1024^2 cfg 3 frame once with depth; then the exchange alone -- direct send of the tiles, ordered over (+ minimum of the
depth), gather on rank 0 -- is timed over K frames through both slots, once on an exchange that carries RGBA only and once
on one that also carries depth.  Prints one line per P and one JSON line with all of it.

The expected cost from the byte count alone is +25 % (20 instead of 16 bytes per pixel per move); that is arithmetic, the
lines below are what is measured.  On one GPU every copy is a device-local copy, so the numbers bound the merge's own
work, not what xGMI links would add between GPUs.

    python tools/shard_depth_time.py [ranks, default 2,4,8] [frames K, default 50]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

pkg = bench.load_package()
RANKS = [int(v) for v in sys.argv[1].split(",")] if len(sys.argv) > 1 else (2, 4, 8)
K = int(sys.argv[2]) if len(sys.argv) > 2 else 50
N, SIZE, PLANES = 128, 1024, 512


def exchange_ms(rs, depth):
    npix = SIZE * SIZE
    xs = [pkg.binding.Exchange(R, r, len(rs), npix) for r, R in enumerate(rs)]
    try:
        pkg.binding.Exchange.connect_local(xs)
        frame = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        dframe = torch.zeros((npix,), dtype=torch.float32, device="cuda")
        for slot in (0, 1):
            for R, x in zip(rs, xs):
                x.acquire(slot)
                R.render_device(x.partial(slot), x.partial_depth(slot) if depth else None, None)
                x.rendered(slot)
        torch.cuda.synchronize()

        def one(i):
            slot = i & 1
            for x in xs:
                x.acquire(slot)
                x.rendered(slot)
            if depth:
                pkg.binding.Exchange.frame_local_depth(xs, slot, frame.data_ptr(), dframe.data_ptr())
            else:
                pkg.binding.Exchange.frame_local(xs, slot, frame.data_ptr())
        for i in range(10):
            one(i)
        xs[0].wait(None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(K):
            one(i)
        xs[0].wait(None)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / K * 1e3
        fin = float(torch.isfinite(dframe).float().mean()) if depth else None
        return ms, fin
    finally:
        for x in xs:
            x.close()


results = []
for P in RANKS:
    rs = []
    try:
        for r in range(P):
            R = pkg.Renderer(0)
            rs.append(R)
            R.set_shard(r, P)
            vghf, nrm = bench.make_volume(R, N)
            R.upload_volume_device(vghf.data_ptr(), (N, N, N), 3, 1, nrm.data_ptr())
            del vghf, nrm
            bench.configure(R, "cfg3", N, SIZE, PLANES)
        torch.cuda.empty_cache()
        ms_rgba, _ = exchange_ms(rs, False)
        ms_depth, fin = exchange_ms(rs, True)
    finally:
        for R in rs:
            R.close()
    row = {"nranks": P, "exchange_ms_rgba": round(ms_rgba, 4), "exchange_ms_rgba_depth": round(ms_depth, 4),
           "measured_increase_pct": round(100.0 * (ms_depth / ms_rgba - 1.0), 1), "bytes_increase_pct_arithmetic": 25.0,
           "depth_finite_fraction": round(fin, 3)}
    results.append(row)
    print("P=%d: exchange %.3f ms RGBA only, %.3f ms RGBA + depth (measured %+.1f %%; bytes +25 %% by arithmetic); %.1f %% of "
          "pixels with a finite depth" % (P, ms_rgba, ms_depth, row["measured_increase_pct"], 100.0 * fin), flush=True)
print(json.dumps({"tool": "shard_depth_time", "frame": [SIZE, SIZE], "volume": N, "frames": K, "results": results}))
