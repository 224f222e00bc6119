"""Times the merge with H on shards beside the one-call entry, and the one-call entry of this build beside another build's, in
one session: python tools/merge_h_shard_time.py [edge] [--parent-lib PATH/libsmk_hip.so]   (edge: default 256)

A 256^3 step, u8 and f32, nelts 4 (V2GH: two fields, G, H), blur 0 and 1.  The method is tools/merge_h_time.py's: HIP events
round batches of calls on one side stream, the median of the windows after warm-up windows, with the smallest and largest.
  (a) smk_merge_timestep_h of the library at --parent-lib (a build of the parent commit), when given;
  (b) smk_merge_timestep_h of this build;
  (c) smk_step_extremes_h_device + smk_merge_timestep_h_shard of this build on an unsharded context, and each alone;
  per rank: the export and the write pass on every rank of 2 and of 8 ranks of one GPU (option halo 3), each rank by itself.
Every library runs in a process of its own (the library is chosen when the package loads), one after the other on the same
GPU, (a) and (b) alternating twice.  Prints a line per row, then all rows as one JSON line.
profiles/step_merge_h_shard.md holds a run."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REP, WARM, BATCH = 9, 3, 4
CODE = {"u8": 0, "f32": 1}
NE, MODE, HALO = 4, "V2GH", 3


def child(section, n):
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    pkg = G._load_package()
    side = torch.cuda.Stream()
    sarg = ctypes.c_void_p(side.cuda_stream)

    def event_ms(work):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        for _ in range(BATCH):
            work()
        b.record(side)
        b.synchronize()
        return a.elapsed_time(b) / BATCH

    def measure(work):
        for _ in range(WARM):
            event_ms(work)
        t = sorted(event_ms(work) for _ in range(REP))
        return statistics.median(t), t[0], t[-1]

    def volume(ring):
        g = torch.Generator(device="cuda").manual_seed(7 + NE)
        z, y, x = torch.meshgrid(*(torch.arange(n, device="cuda", dtype=torch.float32),) * 3, indexing="ij")
        chans = [(torch.sin(x * (.11 + .03 * e)) * .25 + torch.cos(y * .07 + z * (.13 - .02 * e) + e) * .2 + .5 +
                  torch.rand(x.shape, device="cuda", generator=g) * .04) for e in range(NE)]
        v = torch.stack(chans, -1).clamp_(0, 1).contiguous()
        if ring == "u8":
            v = (v * 255).to(torch.uint8).contiguous()
        nrm = torch.randint(0, 256, (n, n, n, 3), dtype=torch.uint8, device="cuda", generator=g)
        return v, nrm

    def context(v, nrm, ring, rank=0, nranks=1):
        R = pkg.Renderer(0)
        try:
            if nranks > 1:
                R.set_shard(rank, nranks)
                R.set_option("halo", HALO)
            R.set_timestep_cache(3)
            R.upload_volume_device(v.data_ptr(), (n, n, n), NE, CODE[ring], nrm.data_ptr(), dmode=MODE)
            torch.cuda.synchronize()
        except Exception:
            R.close()
            raise
        return R

    rows = []

    def row(ring, what, blur, ranks, rank, t):
        rows.append(dict(section=section, ring=ring, what=what, blur=blur, ranks=ranks, rank=rank, ms=t[0], lo=t[1], hi=t[2]))
        print("%-8s %-4s %-34s blur %s ranks %d rank %d  %.3f ms (%.3f - %.3f)" % (section, ring, what, blur, ranks, rank, *t), flush=True)

    for ring in ("u8", "f32"):
        v, nrm = volume(ring)
        R = context(v, nrm, ring)
        try:
            for blur in (0, 1):
                row(ring, "smk_merge_timestep_h", blur, 1, 0, measure(lambda: R.merge_timestep_h(0, 1, 1, 1, blur, stream=sarg)))
            if section == "this":
                w = torch.zeros(8, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                p = w.data_ptr()
                row(ring, "smk_step_extremes_h_device", "-", 1, 0, measure(lambda: R.step_extremes_h_device(0, p, stream=sarg)))
                for blur in (0, 1):
                    row(ring, "smk_merge_timestep_h_shard", blur, 1, 0, measure(lambda: R.merge_timestep_h_shard(0, 1, p, blur=blur, stream=sarg)))

                    def both():
                        R.step_extremes_h_device(0, p, stream=sarg)
                        R.merge_timestep_h_shard(0, 1, p, blur=blur, stream=sarg)
                    row(ring, "export + write", blur, 1, 0, measure(both))
        finally:
            R.close()
        if section == "this":
            for nranks in (2, 8):
                for rank in range(nranks):
                    R = context(v, nrm, ring, rank, nranks)
                    try:
                        w = torch.zeros(8, dtype=torch.int32, device="cuda")
                        torch.cuda.synchronize()
                        p = w.data_ptr()
                        row(ring, "smk_step_extremes_h_device", "-", nranks, rank, measure(lambda: R.step_extremes_h_device(0, p, stream=sarg)))
                        for blur in (0, 1):
                            row(ring, "smk_merge_timestep_h_shard", blur, nranks, rank,
                                measure(lambda: R.merge_timestep_h_shard(0, 1, p, blur=blur, stream=sarg)))
                    finally:
                        R.close()
        del v, nrm
        torch.cuda.empty_cache()
    print("ROWS " + json.dumps(rows), flush=True)


def main():
    args = sys.argv[1:]
    if args and args[0] == "--child":
        return child(args[1], int(args[2]))
    parent = None
    if "--parent-lib" in args:
        i = args.index("--parent-lib")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    n = int(args[0]) if args else 256
    rows = []
    # ("this-again": the one-call rows alone, for the second round of the comparison)
    order = ["parent", "this", "parent", "this-again"] if parent else ["this"]
    for k, section in enumerate(order):
        env = dict(os.environ)
        env.pop("SMK_LIB", None)
        if section == "parent":
            env["SMK_LIB"] = parent
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", section, str(n)], env=env, stdout=subprocess.PIPE, text=True,
                             timeout=600)
        sys.stdout.write("".join(line + "\n" for line in out.stdout.splitlines() if not line.startswith("ROWS ")))
        sys.stdout.flush()
        if out.returncode:
            sys.exit("the %s library's run ended with status %d" % (section, out.returncode))
        for line in out.stdout.splitlines():
            if line.startswith("ROWS "):
                rows += [dict(r, round=k // 2 if parent else 0) for r in json.loads(line[5:])]
    print(json.dumps(dict(n=n, rep=REP, warm=WARM, batch=BATCH, halo=HALO, rows=rows)))


if __name__ == "__main__":
    main()
