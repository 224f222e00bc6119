#!/usr/bin/env python3
"""Developer tool (GPU box): frame times of the three voxel types on the same scenes.

  cfg 3 (512^3 VGH volume, 1024^2 window, 512 planes, R8k shading) as u8, u16 and f32 voxels, brick flags on and off;
  the 1024^3 streaming frame (cfg 4's two tables, 1024^2 x 1024 planes, brick flags off) as u16 and f32 voxels.

Every type renders the SAME data: the f32 VGH volume smk_make_vgh_device makes of the synthetic scalar, its u8 output, and
the f32 output quantised by smk_quantize_u16_device.  Per leg: the settle frames of bench.py (auto mode's trials, the tile
schedule's measured weights), a warm-up, then three series of K frames, each the average HIP-event time of the ray-march kernel alone
(smk_timing_read); the mean of the three and their extremes.  Bytes per step are the stored voxels (what a time step keeps resident and a
streaming frame reads).

With --parent-lib the u8 and f32 legs are run again on that library (the parent commit's build) in the same session, so
the file shows whether existing frames moved.  Each library runs in a child process of its own; this process never opens
the GPU.  The "## Time" section of --md is rewritten, whatever stands before it (the code-object metadata) is kept.

  python tools/u16_time.py [--steps 20] [--parent-lib path/to/libsmk_hip.so] [--md profiles/u16.md] [--no-1024]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DT = {"u8": 0, "f32": 1, "u16": 2}
VOXEL_BYTES = {"u8": 8, "u16": 8, "f32": 16}


def child(a):
    """the legs of one library, as JSON on the last line of stdout"""
    import torch
    import bench
    pkg = bench.load_package()
    r = pkg.Renderer(0)
    types = a.types.split(",")
    rows = []
    work = torch.cuda.Stream()

    def volumes(n):
        dims = (n, n, n)
        scalar = torch.empty(dims, dtype=torch.uint8, device="cuda")
        r.synth_volume_device(1, 1, dims, scalar.data_ptr())
        vgh8 = torch.empty(dims + (3,), dtype=torch.uint8, device="cuda")
        vghf = torch.empty(dims + (3,), dtype=torch.float32, device="cuda")
        r.make_vgh_device(scalar.data_ptr(), 0, dims, 1, vgh8.data_ptr(), vghf.data_ptr())
        nrm = torch.empty(dims + (3,), dtype=torch.uint8, device="cuda")
        r.normals_vgh_device(vgh8.data_ptr(), 3, dims, 0, nrm.data_ptr())
        out = {"u8": vgh8, "f32": vghf, "nrm": nrm}
        if "u16" in types:
            v16 = torch.empty(dims + (3,), dtype=torch.int16, device="cuda")
            r.quantize_u16_device(vghf.data_ptr(), n ** 3 * 3, v16.data_ptr())
            out["u16"] = v16
        del scalar
        return out

    def leg(name, vols, t, n, workload, size, planes, bricks):
        r.upload_volume_device(vols[t].data_ptr(), (n, n, n), 3, DT[t], vols["nrm"].data_ptr())
        bench.configure(r, workload, n, size, planes)
        r.set_option("bricks", bricks)
        frame = torch.empty((size * size, 4), dtype=torch.float32, device="cuda")
        ms = []
        with torch.cuda.stream(work):
            for rep in range(3):      # (three timed series of a.steps frames each: smk_timing_read gives a series' average)
                _, kms, kn = bench.timed(r, a.steps, 3, frame, 1, None, settle=rep == 0)
                ms.append(float(kms))
        kernel = r.last_frame_info()[0]
        rows.append({"scene": name, "type": t, "bricks": bricks, "kernel": {1: "gather", 2: "slice ring"}.get(kernel, str(kernel)),
                     "ms_mean": sum(ms) / len(ms), "ms_min": min(ms), "ms_max": max(ms), "frames": int(kn),
                     "bytes_per_step": n ** 3 * VOXEL_BYTES[t], "slab_failures": r.stat("slab_failures")})
        print(rows[-1], file=sys.stderr, flush=True)
        r.set_option("bricks", 1)
        del frame

    vols = volumes(512)
    for t in types:
        for bricks in (1, 0):
            leg("cfg3 512^3, 1024^2 x 512", vols, t, 512, "cfg3", 1024, 512, bricks)
    del vols
    torch.cuda.empty_cache()
    if not a.no_1024:
        vols = volumes(1024)
        if "u8" in vols and "u8" not in types:
            del vols["u8"]
        for t in [t for t in types if t != "u8"]:
            leg("1024^3 streaming, 1024^2 x 1024", vols, t, 1024, "cfg4", 1024, 1024, 0)
        del vols
    r.close()
    print(json.dumps(rows))


def run_child(a, types, lib=None):
    env = dict(os.environ)
    if lib:
        env["SMK_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--types", types, "--steps", str(a.steps)]
    if a.no_1024:
        cmd.append("--no-1024")
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)      # (stderr: the legs as they finish)
    if p.returncode != 0:
        raise SystemExit("u16_time: the child for %s failed (%d)" % (lib or "this build", p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def table(rows, title):
    out = ["**%s**" % title, "",
           "| scene | voxels | brick flags | kernel (auto mode) | kernel ms: mean of 3 series (min .. max) | frames per series | GB per step |",
           "|---|---|---|---|---|---|---|"]
    for x in rows:
        out.append("| %s | %s | %s | %s | %.3f (%.3f .. %.3f) | %d | %.2f |" % (
            x["scene"], x["type"], "on" if x["bricks"] else "off", x["kernel"], x["ms_mean"], x["ms_min"], x["ms_max"],
            x["frames"], x["bytes_per_step"] / 1e9))
    return out + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--types", default="u8,u16,f32")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libsmk_hip.so: its u8 and f32 legs, same session")
    ap.add_argument("--md", default=None)
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-timeout", type=int, default=420)
    a = ap.parse_args()
    if a.child:
        return child(a)
    mine = run_child(a, a.types)
    lines = ["## Time", "",
             "One MI355X, `tools/u16_time.py --steps %d`: per leg bench.py's settle frames and a warm-up, then three series of %d frames,"
             % (a.steps, a.steps), "each the average HIP-event time of the ray-march kernel (auto mode: the kernel named is the one it kept).  All types",
             "render the same data.", ""]
    lines += table(mine, "This build")
    if a.parent_lib:
        lines += table(run_child(a, "u8,f32", a.parent_lib), "The parent commit's library, same session (u8 and f32 legs)")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.md:
        head = ""
        if os.path.exists(a.md):
            head = open(a.md).read().split("## Time")[0]
        with open(a.md, "w") as f:
            f.write(head + text)


if __name__ == "__main__":
    main()
