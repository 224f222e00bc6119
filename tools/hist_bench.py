#!/usr/bin/env python3
"""Developer tool (GPU box): time the joint histogram (MetaVolume::hist2D's job).

    tools/hist_bench.py [n]                  smk_hist2d_device on an n^3 VGH volume (default 512)
    tools/hist_bench.py --step [n] [out.md]  smk_hist2d_step_device on a resident n^3 step of each voxel type, beside the
                                             raw-array entries on the same volume in the same run (profiles/step_hist.md)
"""
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def raw_array(n):
    pkg = bench.load_package()
    r = pkg.Renderer(0)
    scalar = torch.empty((n, n, n), dtype=torch.uint8, device="cuda")
    r.synth_volume_device(0, 1, (n, n, n), scalar.data_ptr())
    vgh = torch.empty((n, n, n, 3), dtype=torch.uint8, device="cuda")
    r.make_vgh_device(scalar.data_ptr(), 0, (n, n, n), 1, vgh.data_ptr(), None)
    h = r.hist2d_device(vgh.data_ptr(), 3, (n, n, n))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        h = r.hist2d_device(vgh.data_ptr(), 3, (n, n, n))
    dt = (time.perf_counter() - t0) / 5
    print("%d^3 VGH: %.2f ms per histogram (incl. 256 KB read-back + log scaling on the host), %.0f GB/s of voxel bytes; %d non-empty bins"
          % (n, dt * 1e3, 3.0 * n ** 3 / dt / 1e9, int((h > 0).sum())))
    r.close()


def _events(call, stream, warm=3, reps=9):
    """HIP-event times (ms) of `call`, which enqueues on `stream`: median, min, max of `reps` after `warm` calls"""
    ts = []
    for i in range(warm + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        if i >= warm:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


def _wall(call, warm=2, reps=7):
    """host-clock times (ms) of a synchronous entry"""
    ts = []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        if i >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def step(n, out=None):
    pkg = bench.load_package()
    dims = (n, n, n)
    nvox = n ** 3
    gen = pkg.Renderer(0)
    scalar = torch.empty((n, n, n), dtype=torch.uint8, device="cuda")
    gen.synth_volume_device(0, 1, dims, scalar.data_ptr())
    v8 = torch.empty((n, n, n, 3), dtype=torch.uint8, device="cuda")
    vf = torch.empty((n, n, n, 3), dtype=torch.float32, device="cuda")
    gen.make_vgh_device(scalar.data_ptr(), 0, dims, 1, v8.data_ptr(), vf.data_ptr())
    v16 = torch.empty((n, n, n, 3), dtype=torch.int16, device="cuda")
    gen.quantize_u16_device(vf.data_ptr(), 3 * nvox, v16.data_ptr())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    sarg = ctypes.c_void_p(s.cuda_stream)
    cnt = torch.zeros(65536, dtype=torch.int32, device="cuda")
    rows = []
    for name, dt, vol, stored, raw_bytes in (("u8", 0, v8, 8, 3), ("f32", 1, vf, 16, 12), ("u16", 2, v16, 8, None)):
        r = pkg.Renderer(0)
        r.upload_volume_device(vol.data_ptr(), dims, 3, dt)
        ev = _events(lambda: r.hist2d_step_device(cnt.data_ptr(), stream=sarg), s)
        counts = cnt.cpu().numpy().view(np.uint32).reshape(256, 256)
        assert int(counts.astype(np.int64).sum()) == nvox
        host = _wall(lambda: r.hist2d_step(want="hist"))
        raw = None
        if raw_bytes:
            entry = r.hist2d_device if dt == 0 else r.hist2d_f32_device
            raw = _wall(lambda: entry(vol.data_ptr(), 3, dims))
            assert np.array_equal(entry(vol.data_ptr(), 3, dims), pkg.Renderer.hist2d_finish(counts)), name
        rows.append((name, stored * nvox, ev, host, raw, raw_bytes and raw_bytes * nvox, int((counts > 0).sum())))
        r.close()
    gen.close()
    lines = ["| voxels | stored bytes | `smk_hist2d_step_device`, HIP events, ms | TB/s of stored bytes | Gvoxel/s | `smk_hist2d_step` to host bytes, wall ms | raw-array entry, wall ms | its array | non-empty bins |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, sb, ev, host, raw, rb, bins in rows:
        lines.append("| %s | %d MiB | %.3f (min %.3f, max %.3f) | %.2f | %.0f | %.3f (min %.3f, max %.3f) | %s | %s | %d |" % (
            name, sb >> 20, ev[0], ev[1], ev[2], sb / ev[0] / 1e9, nvox / ev[0] / 1e6, host[0], host[1], host[2],
            "%.3f (min %.3f, max %.3f)" % raw if rb else "none", "%d MiB" % (rb >> 20) if rb else "-", bins))
    text = "\n".join(lines)
    print("%d^3 VGH step, 3 channels; events: median of 9 after 3 warm-up calls on a stream of the caller's; wall: median of 7 after 2" % n)
    print(text)
    if out:
        open(out, "w").write("%d^3\n\n%s\n" % (n, text))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--step":
        step(int(args[1]) if len(args) > 1 else 512, args[2] if len(args) > 2 else None)
    else:
        raw_array(int(args[0]) if args else 512)


if __name__ == "__main__":
    main()
