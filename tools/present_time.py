#!/usr/bin/env python3
"""Wall-clock time per DELIVERED frame of the cfg 3 frame (512^3 f32 VGH, 1024^2 x 512, built as bench.py builds it) on the
three ways a host can take it (developer tool, GPU box only; DESIGN.md 5 "Present"):
  (a) smk_render into a (preallocated, touched) numpy array: float RGBA to pageable memory -- the path before the present
      entries, still in the tree unchanged, hence the baseline;
  (b) smk_render_present: RGBA8 into the context's pinned buffers, synchronous;
  (c) smk_render_present_begin / _end with two frames in flight: frame k's copy beside frame k + 1's ray-march.
Per case: the median over all timed frames (FRAMES per round, ROUNDS rounds, the cases taken in turn within a round so that
whatever else the machine does meets all three alike), the per-round medians as the spread, the kernel time of
smk_last_frame_info, present_ms and the bytes copied.  Also the two copies on their own (torch, HIP events): 16 MiB to
pageable memory, 4 MiB to pinned memory.  One process; it ends itself after --limit seconds.
    timeout -k 10 900 python tools/present_time.py [--volume 512] [--frames 60] [--rounds 3] [--out profiles/r05_present.md]"""
import argparse
import ctypes as C
import os
import signal
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

SIZE, PLANES = 1024, 512
BG = (1.0, 1.0, 1.0)   # gluvv.env.bgColor == 0


def case_a(r, n, buf):
    """smk_render into a numpy array"""
    per, kms = [], []
    p = buf.ctypes.data_as(C.c_void_p)
    for _ in range(n):
        t0 = time.perf_counter()
        r._ck(r.L.smk_render(r.ctx, p, None))
        per.append((time.perf_counter() - t0) * 1e3)
        kms.append(r.last_frame_info()[1])
    return per, kms, [], buf.nbytes


def case_b(r, n, _):
    per, kms, pms = [], [], []
    for _ in range(n):
        t0 = time.perf_counter()
        r.render_present(bg=BG, copy=False)
        per.append((time.perf_counter() - t0) * 1e3)
        kms.append(r.last_frame_info()[1])
        pms.append(r.stat("present_ms"))
    return per, kms, pms, r.stat("present_bytes")


def case_c(r, n, _):
    """two frames in flight: begin k + 1, then end k; one delivered frame per turn"""
    per, kms, pms = [], [], []
    prev = r.render_present_begin(bg=BG)
    for _ in range(n):
        t0 = time.perf_counter()
        t = r.render_present_begin(bg=BG)
        r.render_present_end(prev)
        per.append((time.perf_counter() - t0) * 1e3)
        kms.append(r.last_frame_info()[1])
        pms.append(r.stat("present_ms"))
        prev = t
    r.render_present_end(prev)
    return per, kms, pms, r.stat("present_bytes")


def copies_alone(reps=30):
    """the two device-to-host copies on an idle device, HIP events: (16 MiB float frame -> pageable, 4 MiB RGBA8 -> pinned) ms"""
    d16 = torch.zeros(SIZE * SIZE * 4, dtype=torch.float32, device="cuda")
    d4 = torch.zeros(SIZE * SIZE, dtype=torch.int32, device="cuda")
    h16 = torch.zeros(SIZE * SIZE * 4, dtype=torch.float32)
    h4 = torch.zeros(SIZE * SIZE, dtype=torch.int32).pin_memory()
    out = []
    for dst, src in ((h16, d16), (h4, d4)):
        ms = []
        for _ in range(reps + 5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out.append(float(np.median(ms[5:])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=int, default=840, help="seconds after which the process ends itself")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    signal.alarm(a.limit)
    if not torch.cuda.is_available():
        sys.exit("present_time: no GPU (nothing is measured on the CPU)")
    n = a.volume
    pkg = bench.load_package()
    r = pkg.Renderer(0)
    vghf, nrm = bench.make_volume(r, n)
    r.upload_volume_device(vghf.data_ptr(), (n, n, n), 3, 1, nrm.data_ptr())
    del vghf, nrm
    bench.configure(r, "cfg3", n, SIZE, PLANES)
    buf = np.ones((SIZE, SIZE, 4), np.float32)
    cases = (("a", "smk_render -> numpy (float RGBA, pageable)", case_a),
             ("b", "smk_render_present (RGBA8, pinned, synchronous)", case_b),
             ("c", "begin / end, two frames in flight", case_c))
    warm = bench.SETTLE_FRAMES + 8
    for _, _, f in cases:      # auto mode measures each configuration's kernels first; pinned buffers are made
        f(r, warm, buf)
    res = {k: {"per": [], "rounds": [], "kms": [], "pms": [], "bytes": 0} for k, _, _ in cases}
    for _ in range(a.rounds):
        for k, _, f in cases:
            f(r, 5, buf)
            per, kms, pms, nbytes = f(r, a.frames, buf)
            res[k]["per"] += per
            res[k]["rounds"].append(float(np.median(per)))
            res[k]["kms"] += kms
            res[k]["pms"] += pms
            res[k]["bytes"] = nbytes
    kernel = r.last_frame_info()[0]
    failures, retries = r.stat("slab_failures"), r.stat("slab_retries")
    r.close()
    c16, c4 = copies_alone()
    med = {k: float(np.median(v["per"])) for k, v in res.items()}
    lines = ["# Time per delivered frame: cfg 3, %d^3 f32 VGH, %d^2 x %d (tools/present_time.py)" % (n, SIZE, PLANES), "",
             "Wall clock around each call (every call ends in a wait for the frame's bytes), median of %d frames per case: %d rounds"
             % (a.frames * a.rounds, a.rounds),
             "of %d, the three cases in turn within a round, after %d warm-up frames each.  Kernel: HIP events round the ray-marcher"
             % (a.frames, warm),
             "(smk_last_frame_info; kernel %d).  slab_failures %d, slab_retries %d." % (kernel, failures, retries), "",
             "| case | ms / delivered frame (median) | per-round medians | frames / s | kernel ms | present_ms | bytes to host |",
             "|---|---|---|---|---|---|---|"]
    for k, name, _ in cases:
        v = res[k]
        lines.append("| (%s) %s | %.3f | %s | %.0f | %.3f | %s | %d |" % (
            k, name, med[k], ", ".join("%.3f" % x for x in v["rounds"]), 1e3 / med[k], float(np.median(v["kms"])),
            "%.4f" % float(np.median(v["pms"])) if v["pms"] else "-", v["bytes"]))
    kms = float(np.median(res["c"]["kms"]))
    lines += ["", "The copies alone, idle device, host clock round copy + synchronise: 16 MiB float frame to pageable memory %.3f ms; "
              "4 MiB RGBA8 to pinned memory %.3f ms." % (c16, c4), "",
              "(c) against its bound: max(kernel %.3f, pinned copy %.3f) = %.3f ms; measured %.3f ms (%.2fx the bound)."
              % (kms, c4, max(kms, c4), med["c"], med["c"] / max(kms, c4)),
              "(c) against (a): %.2fx the delivered frame rate; (b) against (a): %.2fx." % (med["a"] / med["c"], med["a"] / med["b"])]
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
