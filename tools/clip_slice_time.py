#!/usr/bin/env python3
"""Cost of the clip-plane widget's data slice (smk_set_clip_slice) on the cfg 3 frame (developer tool, GPU box only):
  (a) the frame time with the slice off (HIP events round the render kernels, repeated windows: mean and spread);
  (b) a quad that covers the whole 1024^2 window: the frame with the slice on, and smk_render_slice_device for the same
      quad and window called behind every frame's ray-marcher.  Run under `rocprofv3 --kernel-trace --stats`: the two
      kernels' own times are in the kernel statistics (smk_k_clip_slice, smk_k_render_slice).
A library without smk_set_clip_slice (SMK_LIB=<an older build>) runs what it has.
    python tools/clip_slice_time.py [volume] [repeats]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402

SIZE, PLANES, FRAMES = 1024, 512, 20


def windows(r, frame, st, repeats):
    """`repeats` windows of FRAMES frames: the average kernel time of each (ms)"""
    out = []
    for _ in range(repeats):
        r.timing_reset()
        for _ in range(FRAMES):
            r.render_device(frame.data_ptr(), None, st)
        torch.cuda.synchronize()
        out.append(r.timing_read()[0])
    return out


def stats(v):
    return {"mean_ms": float(np.mean(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "n": len(v)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    pkg = bench.load_package()
    r = pkg.Renderer(0)
    have = hasattr(r.L, "smk_set_clip_slice") and not type(r.L.smk_set_clip_slice).__name__ == "_Missing"
    vghf, nrm = bench.make_volume(r, n)
    r.upload_volume_device(vghf.data_ptr(), (n, n, n), 3, 1, nrm.data_ptr())
    del vghf, nrm
    bench.configure(r, "cfg3", n, SIZE, PLANES)
    frame = torch.zeros((SIZE * SIZE, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    res = {"library": pkg.library_path(), "volume": n, "has_clip_slice": bool(have)}
    # (a) the headline frame, slice off (auto mode settles first)
    for _ in range(bench.SETTLE_FRAMES + 8):
        r.render_device(frame.data_ptr(), None, st)
    torch.cuda.synchronize()
    res["cfg3_frame_slice_off"] = stats(windows(r, frame, st, repeats))
    res["cfg3_kernel"] = r.last_frame_info()[0]
    # (b) view along z, a Z+ plane nearer than the volume's centre: its cut face is wider than the window
    ident = [1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    r.set_camera(bench.modelview(np.eye(4), (1.0, 1.0, 1.0)), bench.FRUSTUM, (1.0, 20.0), SIZE, SIZE)
    r.set_shading("r8k", bench.LIGHT, bench.EYE, bench.AT, ident, bench.INTENS)
    vpos = (0.5, 0.5, 0.4)
    r.set_clip(5, vpos)
    corners = np.array([[-.2, -.2, .4], [1.2, -.2, .4], [1.2, 1.2, .4], [-.2, 1.2, .4]], np.float32)
    moved = np.clip(corners, 0, 1)
    moved[:, 2] += np.float32(.001)
    for _ in range(bench.SETTLE_FRAMES + 8):
        r.render_device(frame.data_ptr(), None, st)
    torch.cuda.synchronize()
    off = windows(r, frame, st, repeats)
    res["zview_frame_slice_off"] = stats(off)
    base = frame.clone()
    if have:
        for dv, name in ((-0.5, "before"), (0.5, "after")):
            r.set_clip_slice(corners, 0.6, dv, "r8k")
            for _ in range(8):
                r.render_device(frame.data_ptr(), None, st)
            torch.cuda.synchronize()
            on = windows(r, frame, st, repeats)
            res["zview_frame_slice_" + name] = stats(on)
            res["slice_pass_%s_by_difference_ms" % name] = float(np.mean(on) - np.mean(off))
            res["pixels_changed_" + name] = int(((frame - base).abs().amax(dim=1) > 0).sum())
        r.set_clip_slice(None)
    # smk_render_slice_device for the same quad and window, in the same place: behind every frame's ray-marcher, on the
    # frame it has just written (a slice drawn over and over on its own would find frame and voxels in the caches)
    q = np.ascontiguousarray(moved, np.float32).reshape(12)
    import ctypes as C
    qp = q.ctypes.data_as(C.POINTER(C.c_float))
    per_pair = []
    for rep in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(FRAMES):
            r.render_device(frame.data_ptr(), None, st)
            r._ck(r.L.smk_render_slice_device(r.ctx, qp, 0.6, frame.data_ptr(), st))
        e1.record()
        torch.cuda.synchronize()
        per_pair.append(e0.elapsed_time(e1) / FRAMES)
    res["zview_frame_then_render_slice_wall"] = stats(per_pair)
    print(json.dumps(res), flush=True)
    r.close()


if __name__ == "__main__":
    main()
