"""Times smk_merge_timestep_h beside smk_merge_timestep and smk_derive_timestep in one session: python tools/merge_h_time.py [edge]
(default 256); prints a line per entry, then all of them as one JSON line.  profiles/step_merge_h.md holds a run."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

pkg = G._load_package()
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
REP, WARM, BATCH = 9, 3, 4
CODE = {"u8": 0, "f32": 1}


def event_ms(stream, work):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(BATCH):
        work()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / BATCH


def measure(stream, work):
    for _ in range(WARM):
        event_ms(stream, work)
    t = sorted(event_ms(stream, work) for _ in range(REP))
    return statistics.median(t), t[0], t[-1]


def volume(ring, ne):
    g = torch.Generator(device="cuda").manual_seed(7 + ne)
    z, y, x = torch.meshgrid(*(torch.arange(N, device="cuda", dtype=torch.float32),) * 3, indexing="ij")
    chans = [(torch.sin(x * (.11 + .03 * e)) * .25 + torch.cos(y * .07 + z * (.13 - .02 * e) + e) * .2 + .5 +
              torch.rand(x.shape, device="cuda", generator=g) * .04) for e in range(ne)]
    v = torch.stack(chans, -1).clamp_(0, 1).contiguous()
    if ring == "u8":
        v = (v * 255).to(torch.uint8).contiguous()
    nrm = torch.randint(0, 256, (N, N, N, 3), dtype=torch.uint8, device="cuda", generator=g)
    return v, nrm


rows = []
side = torch.cuda.Stream()
import ctypes  # noqa: E402
sarg = ctypes.c_void_p(side.cuda_stream)
for ring in ("u8", "f32"):
    for ne, mode in ((4, "V2GH"), (3, "V2G")):
        v, nrm = volume(ring, ne)
        R = pkg.Renderer(0)
        try:
            R.set_timestep_cache(3)
            R.upload_volume_device(v.data_ptr(), (N, N, N), ne, CODE[ring], nrm.data_ptr(), dmode=mode)
            torch.cuda.synchronize()
            vox = 8 if ring == "u8" else 16
            cases = []
            if ne == 4:
                cases += [("merge_timestep_h add_h 1 blur 0 (nf 2)", lambda: R.merge_timestep_h(0, 1, 1, 1, 0, stream=sarg)),
                          ("merge_timestep_h add_h 1 blur 1 (nf 2)", lambda: R.merge_timestep_h(0, 1, 1, 1, 1, stream=sarg)),
                          ("merge_timestep (nf 3)", lambda: R.merge_timestep(0, 1, stream=sarg))]
            else:
                cases += [("merge_timestep (nf 2)", lambda: R.merge_timestep(0, 1, stream=sarg)),
                          ("merge_timestep_h add_h 0 blur 0 (nf 2)", lambda: R.merge_timestep_h(0, 1, 0, 1, 0, stream=sarg)),
                          ("merge_timestep_h add_h 0 blur 1 (nf 2)", lambda: R.merge_timestep_h(0, 1, 0, 1, 1, stream=sarg)),
                          ("derive_timestep blur 0", lambda: R.derive_timestep(0, 1, 1, 0, stream=sarg)),
                          ("derive_timestep blur 1", lambda: R.derive_timestep(0, 1, 1, 1, stream=sarg))]
            for name, work in cases:
                med, lo, hi = measure(side, work)
                nbytes = N ** 3 * (3 * vox + (4 if (ring == "f32" and ne == 4) else 0))   # two reads of the source, one write
                rows.append(dict(ring=ring, nelts=ne, entry=name, ms=med, lo=lo, hi=hi, gbs=nbytes / med / 1e6))
                print("%-4s nelts %d  %-42s %.3f ms (%.3f - %.3f)  %.0f GB/s" % (ring, ne, name, med, lo, hi, nbytes / med / 1e6), flush=True)
        finally:
            R.close()
        del v, nrm
        torch.cuda.empty_cache()
print(json.dumps(dict(n=N, rep=REP, warm=WARM, batch=BATCH, rows=rows)))
