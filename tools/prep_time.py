#!/usr/bin/env python3
"""Developer tool (GPU box): time the data-preparation entries on n^3 volumes.

  genvol spheres + blur (smk_synth_volume_device kind 1), one timed call per size, as before
  normals / merge / histogram: the u8 entries and their float siblings in one run, on the VGH volume that
  smk_make_vgh_device makes of the synthetic scalar (its u8 and its f32 output), HIP events around each call
  (every entry synchronises before it returns, so this is what a caller waits for: launches, the merge's and the
  histogram's device allocation and the histogram's 256 KB read-back and host finish included), warm-up calls first,
  the median of the timed ones.  Bytes are algorithmic: every input element read once per pass over the volume
  (interleaved channels come with their cache line whether the entry uses them or not), every output element
  written once.

  python tools/prep_time.py [--n 512] [--runs 20] [--genvol 512,1024] [--md out.md]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402


def genvol(r, sizes):
    for n in sizes:
        out = torch.empty((n, n, n), dtype=torch.uint8, device="cuda")
        r.synth_volume_device(1, 1, (n, n, n), out.data_ptr())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.synth_volume_device(1, 1, (n, n, n), out.data_ptr())
        torch.cuda.synchronize()
        print("genvol spheres+blur %d^3: %.2f ms" % (n, (time.perf_counter() - t0) * 1e3), flush=True)
        del out


def timed(call, runs, warmup=3):
    """median and extremes (ms) of `runs` calls between HIP events, after `warmup` calls"""
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def prep_entries(r, n, runs):
    dims, nv = (n, n, n), n ** 3
    scalar = torch.empty((n, n, n), dtype=torch.uint8, device="cuda")
    r.synth_volume_device(0, 1, dims, scalar.data_ptr())
    vgh8 = torch.empty((n, n, n, 3), dtype=torch.uint8, device="cuda")
    vghf = torch.empty((n, n, n, 3), dtype=torch.float32, device="cuda")
    r.make_vgh_device(scalar.data_ptr(), 0, dims, 1, vgh8.data_ptr(), vghf.data_ptr())
    two8, twof, onef = vgh8[..., :2].contiguous(), vghf[..., :2].contiguous(), vghf[..., :1].contiguous()
    nrm = torch.empty((n, n, n, 3), dtype=torch.uint8, device="cuda")
    out8 = torch.empty((n, n, n, 3), dtype=torch.uint8, device="cuda")
    outf = torch.empty((n, n, n, 3), dtype=torch.float32, device="cuda")
    del scalar
    p = lambda t: t.data_ptr()  # noqa: E731
    # (name, call, algorithmic bytes)
    rows = [
        ("normals u8, 3 channels", lambda: r.normals_vgh_device(p(vgh8), 3, dims, 0, p(nrm)), (3 + 3) * nv),
        ("normals f32, 3 channels", lambda: r.normals_f32_device(p(vghf), 3, dims, 0, p(nrm)), (12 + 3) * nv),
        ("normals f32, 1 channel", lambda: r.normals_f32_device(p(onef), 1, dims, 0, p(nrm)), (4 + 3) * nv),
        ("normals u8, 3 channels, blur", lambda: r.normals_vgh_device(p(vgh8), 3, dims, 1, p(nrm)), (3 + 3) * nv),
        ("normals f32, 3 channels, blur", lambda: r.normals_f32_device(p(vghf), 3, dims, 1, p(nrm)), (12 + 3) * nv),
        ("normals f32, 1 channel, blur", lambda: r.normals_f32_device(p(onef), 1, dims, 1, p(nrm)), (4 + 3) * nv),
        # two passes over the fields (maximum, then write), fields + G and the normals out
        ("merge u8, 2 fields + normals", lambda: r.merge_fields_device(p(two8), 2, dims, p(out8), p(nrm)),
         (2 * 2 + 3 + 3) * nv),
        ("merge f32, 2 fields + normals", lambda: r.merge_fields_f32_device(p(twof), 2, dims, p(outf), p(nrm)),
         (2 * 8 + 12 + 3) * nv),
        ("hist2d u8, 3 channels", lambda: r.hist2d_device(p(vgh8), 3, dims), 3 * nv),
        ("hist2d f32, 3 channels", lambda: r.hist2d_f32_device(p(vghf), 3, dims), 12 * nv),
    ]
    lines = ["| entry at %d^3 | call time: median ms (min .. max of %d) | algorithmic MB | algorithmic GB/s of the call |" % (n, runs),
             "|---|---|---|---|"]
    for name, call, nbytes in rows:
        med, lo, hi = timed(call, runs)
        lines.append("| %s | %.3f (%.3f .. %.3f) | %.0f | %.0f |" % (name, med, lo, hi, nbytes / 1e6, nbytes / med / 1e6))
        print(lines[-1], flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--genvol", default="512,1024", help="sizes of the genvol timing, comma separated; empty = skip")
    ap.add_argument("--md", default=None, help="also write the table to this file")
    a = ap.parse_args()
    pkg = bench.load_package()
    r = pkg.Renderer(0)
    genvol(r, [int(s) for s in a.genvol.split(",") if s])
    lines = prep_entries(r, a.n, a.runs)
    if a.md:
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")
    r.close()


if __name__ == "__main__":
    main()
