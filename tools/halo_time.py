"""Times the halo refill on one GPU: python tools/halo_time.py [edge] [halo]      (defaults: 256, 24)

8 shard contexts of one device hold an edge^3 series (f32 with three channels: 16-byte voxels; u8: 8-byte voxels) with option
halo 24.  HIP events round single calls on one side stream; the median of REP windows after WARM warm-up windows, with the
smallest and the largest.  Per ring:
  exports   smk_step_halo_exports_device, every rank in turn (bytes: the rank's total_send)
  entries   smk_step_halo_entries_device, every rank in turn (bytes: the rank's total_recv): the scatter AND the brick
            summaries of the whole stored box
  local     smk_step_halo_exchange_local of all 8 ranks on the one stream (bytes: the sum of total_recv, read once and
            written once), summaries included
  copy3d    the boxes of `local`, between buffers of the slots' sizes, each as one hipMemcpy3DAsync: the runtime's own figure
            for the same copies, without summaries
  kernels   the device time of smk_k_halo_boxes and smk_k_brick_minmax inside one more `local`, from torch's profiler when it
            records kernels of a foreign library (else absent): the split of scatter and summaries
GB/s counts the bytes once (moved), not read + written.  Transport between devices is not measured: one GPU.
Prints a line per row, then all rows as one JSON line.  profiles/step_halo.md holds a run."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REP, WARM, NRANKS = 21, 5, 8
CODE = {"u8": 0, "f32": 1}
VB = {"u8": 8, "f32": 16}


class Pos(ctypes.Structure):
    _fields_ = [("x", ctypes.c_size_t), ("y", ctypes.c_size_t), ("z", ctypes.c_size_t)]


class PitchedPtr(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("pitch", ctypes.c_size_t), ("xsize", ctypes.c_size_t), ("ysize", ctypes.c_size_t)]


class Extent(ctypes.Structure):
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("depth", ctypes.c_size_t)]


class Memcpy3DParms(ctypes.Structure):
    _fields_ = [("srcArray", ctypes.c_void_p), ("srcPos", Pos), ("srcPtr", PitchedPtr), ("dstArray", ctypes.c_void_p), ("dstPos", Pos),
                ("dstPtr", PitchedPtr), ("extent", Extent), ("kind", ctypes.c_int)]


DEVICE_TO_DEVICE = 3  # hipMemcpyDeviceToDevice


def boxes_of(pkg, dims, halo, ring):
    """per rank (g0, g1, O, D): the region and the stored box, smk_volume_geometry's rule"""
    out = []
    for r in range(NRANKS):
        g0, g1 = pkg.sortlast.shard_region(dims, r, NRANKS)
        O = [max(g0[a] - halo, 0) for a in range(3)]
        D = [min(g1[a] + halo, dims[a]) - O[a] for a in range(3)]
        if ring != "f32":
            for a in range(2):
                if D[a] & 1:
                    if O[a] + D[a] < dims[a]:
                        D[a] += 1
                    elif O[a] > 0:
                        O[a] -= 1
                        D[a] += 1
                    else:
                        D[a] += 1
        out.append((g0, g1, O, D))
    return out


def main():
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    pkg = G._load_package()
    from simian_spacemonkey_amd import sortlast
    pkg.sortlast = sortlast
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    halo = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    dims = (n, n, n)
    side = torch.cuda.Stream()
    sarg = ctypes.c_void_p(side.cuda_stream)
    torch.cuda.init()
    # the HIP runtime this process already runs on (a second copy would not know the side stream)
    with open("/proc/self/maps") as maps:
        loaded = sorted({line.split()[-1] for line in maps if "libamdhip64.so" in line})
    if len(loaded) != 1:
        sys.exit("expected one loaded libamdhip64.so, found %s" % loaded)
    hip = ctypes.CDLL(loaded[0])
    hip.hipMemcpy3DAsync.argtypes = [ctypes.POINTER(Memcpy3DParms), ctypes.c_void_p]
    hip.hipMemcpy3DAsync.restype = ctypes.c_int

    def event_ms(work):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        work()
        b.record(side)
        b.synchronize()
        return a.elapsed_time(b)

    def measure(work):
        for _ in range(WARM):
            event_ms(work)
        t = sorted(event_ms(work) for _ in range(REP))
        return statistics.median(t), t[0], t[-1]

    rows = []

    def row(ring, what, rank, nbytes, t):
        gbs = nbytes / (t[0] * 1e-3) / 1e9 if t[0] > 0 else 0.0
        rows.append(dict(ring=ring, what=what, rank=rank, bytes=nbytes, ms=t[0], lo=t[1], hi=t[2], gbs=gbs))
        print("%-4s %-10s rank %2d  %11d bytes  %.4f ms (%.4f - %.4f)  %.1f GB/s" % (ring, what, rank, nbytes, *t, gbs), flush=True)

    for ring in ("f32", "u8"):
        g = torch.Generator(device="cuda").manual_seed(5)
        if ring == "f32":
            v = torch.rand((n, n, n, 3), device="cuda", generator=g)
        else:
            v = torch.randint(0, 256, (n, n, n, 3), dtype=torch.uint8, device="cuda", generator=g)
        nrm = torch.randint(0, 256, (n, n, n, 3), dtype=torch.uint8, device="cuda", generator=g)
        torch.cuda.synchronize()
        rs = []
        try:
            for r in range(NRANKS):
                R = pkg.Renderer(0)
                rs.append(R)
                R.set_shard(r, NRANKS)
                R.set_option("halo", halo)
                R.set_timestep_cache(2)
                R.upload_volume_device(v.data_ptr(), dims, 3, CODE[ring], nrm.data_ptr(), dmode="VGH")
            torch.cuda.synchronize()
            del v, nrm
            lay = [R.step_halo_layout(NRANKS) for R in rs]
            for r, R in enumerate(rs):
                buf = torch.zeros((max(lay[r][2], lay[r][3]),), dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                p = buf.data_ptr()
                row(ring, "exports", r, lay[r][2], measure(lambda: R.step_halo_exports_device(p, 0, sarg)))
                # (its own exports as entries: the same bytes moved; the segments are not validated, and the halo is made whole below)
                row(ring, "entries", r, lay[r][3], measure(lambda: R.step_halo_entries_device(p, 0, sarg)))
                del buf
            total = sum(l[3] for l in lay)
            row(ring, "local", -1, total, measure(lambda: sortlast.refill_halo_local(rs, 0, stream=sarg)))
            # the same boxes by the runtime's 3-D copy, between buffers of the slots' sizes
            bx = boxes_of(pkg, dims, halo, ring)
            slots = [torch.zeros((D[0] * D[1] * D[2] * VB[ring],), dtype=torch.uint8, device="cuda") for _, _, _, D in bx]
            parms, moved = [], 0
            for j, (_, _, Oj, Dj) in enumerate(bx):
                for i, (g0, g1, Oi, Di) in enumerate(bx):
                    if i == j:
                        continue
                    lo = [max(g0[a], Oj[a]) for a in range(3)]
                    hi = [min(g1[a], min(Oj[a] + Dj[a], dims[a])) for a in range(3)]
                    if any(h <= l for l, h in zip(lo, hi)):
                        continue
                    P = Memcpy3DParms()
                    P.srcPos = Pos((lo[0] - Oi[0]) * VB[ring], lo[1] - Oi[1], lo[2] - Oi[2])
                    P.srcPtr = PitchedPtr(slots[i].data_ptr(), Di[0] * VB[ring], Di[0] * VB[ring], Di[1])
                    P.dstPos = Pos((lo[0] - Oj[0]) * VB[ring], lo[1] - Oj[1], lo[2] - Oj[2])
                    P.dstPtr = PitchedPtr(slots[j].data_ptr(), Dj[0] * VB[ring], Dj[0] * VB[ring], Dj[1])
                    P.extent = Extent((hi[0] - lo[0]) * VB[ring], hi[1] - lo[1], hi[2] - lo[2])
                    P.kind = DEVICE_TO_DEVICE
                    parms.append(P)
                    moved += (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) * VB[ring]
            torch.cuda.synchronize()

            def copies():
                for P in parms:
                    rc = hip.hipMemcpy3DAsync(ctypes.byref(P), sarg)
                    if rc:
                        raise RuntimeError("hipMemcpy3DAsync failed: %d" % rc)
            row(ring, "copy3d", -1, moved, measure(copies))
            del slots
            # the split of the local form into its kernels
            try:
                from torch.profiler import profile, ProfilerActivity
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    sortlast.refill_halo_local(rs, 0, stream=sarg)
                    torch.cuda.synchronize()
                for ev in prof.key_averages():
                    for name in ("smk_k_halo_boxes", "smk_k_brick_minmax"):
                        if name in ev.key:
                            dt = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
                            t = dt / 1e3
                            row(ring, "kernels:" + name, -1, total if "halo" in name else 0, (t, t, t))
            except Exception as e:  # (a profiler without kernel records: the split stays unmeasured)
                print("the profiler gave no kernel times: %s" % e, flush=True)
        finally:
            for R in rs:
                R.close()
        torch.cuda.empty_cache()
    print(json.dumps(dict(n=n, halo=halo, ranks=NRANKS, rep=REP, warm=WARM, rows=rows)))


if __name__ == "__main__":
    main()
