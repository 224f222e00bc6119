#!/usr/bin/env python3
"""Kernel times of the cfg 3 frame with shadows on P shard contexts that share ONE GPU, P = 1 / 2 / 4 / 8 (developer tool, GPU
box only).  Per rank: phase 1 (smk_shadow_exports_device) and the frame (smk_render_device: phase 2's light march + the
eye pass; a whole-volume context at P = 1 marches without phase 1), HIP-event times on one stream, median of a few frames.
The ranks run one after another on one device: this is the cost of each rank's share measured with P contexts on one GPU,
not a scaling curve across GPUs.  Under `rocprofv3 --kernel-trace --stats -- python tools/shadow_shard_time.py` the stats
split the frame into smk_k_shadow_light_march and the eye-pass kernel.
    python tools/shadow_shard_time.py [volume] [light buffer px] [frames]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def make_ranks(pkg, n, lb, world):
    vghf, nrm = None, None
    rs = []
    for r in range(world):
        halo = 4
        while True:
            R = pkg.Renderer(0)
            if world > 1:
                R.set_shard(r, world)
                R.set_option("halo", halo)
            if vghf is None:
                vghf, nrm = bench.make_volume(R, n)
            R.upload_volume_device(vghf.data_ptr(), (n, n, n), 3, 1, nrm.data_ptr())
            xform, _ = bench.configure(R, "cfg3", n, 1024, 512)
            R.set_shading("r8k", (3.0, 4.0, -3.0), bench.EYE, bench.AT, [float(v) for v in xform.T.reshape(-1)], bench.INTENS)
            R.set_shadow(1, lb, 0.5)
            need = R.shadow_margin()[1] if world > 1 else 0
            if need <= halo:
                break
            R.close()
            halo = need
        rs.append(R)
    del vghf, nrm
    return rs


def ms(fn, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    lb = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    frames = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    pkg = bench.load_package()
    frame = torch.zeros((1024 * 1024, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()            # (a stream of its own: the default stream's handle is NULL, which the calls read as
                                        #  "the context's stream")
    print("measured on ONE GPU with P contexts (ranks one after another), not across GPUs; median of %d frames" % frames, flush=True)
    for world in (1, 2, 4, 8):
        rs = make_ranks(pkg, n, lb, world)
        try:
            LB = rs[0].shadowcoef().LB
            exports = torch.zeros((world, world, LB, LB, 4), dtype=torch.float32, device="cuda")
            t1 = [[] for _ in rs]
            t2 = [[] for _ in rs]
            warm = 12                     # (auto mode's kernel trials: the first frames of a configuration)
            for f in range(frames + warm):
                if world > 1:
                    for r, R in enumerate(rs):
                        t = ms(lambda: R.shadow_exports_device(exports[r].data_ptr(), st.cuda_stream), st)
                        if f >= warm:
                            t1[r].append(t)
                    entries = exports.transpose(0, 1).contiguous()
                    for j, R in enumerate(rs):
                        R.shadow_entries_device(entries[j].data_ptr(), st.cuda_stream)
                for r, R in enumerate(rs):
                    t = ms(lambda: R.render_device(frame.data_ptr(), None, st.cuda_stream), st)
                    if f >= warm:
                        t2[r].append(t)
            for r in range(world):
                p1 = "%.3f" % statistics.median(t1[r]) if t1[r] else "-"
                print("P=%d rank %d  phase 1 %s ms  frame (phase 2 + eye pass) %.3f ms  halo %s" % (
                    world, r, p1, statistics.median(t2[r]), rs[r].shadow_margin()[1] if world > 1 else "-"), flush=True)
        finally:
            for R in rs:
                R.close()
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
