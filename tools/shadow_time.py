#!/usr/bin/env python3
"""Frame time of the cfg 3 frame with shadows: the two marches (default) against a launch per slice (developer tool, GPU
box only).   python tools/shadow_time.py [volume] [light buffer px] [--perturb] [--look=0|1]
--perturb: the same frame with the perturbed fetch on (option shadow_perturb; createNoiseTex's 32^3 texture, the two live
octaves at weights (.2, .1), scales (.2, 2.1)): the eye pass is the gather kernel's -- the slice-ring kernel declines
perturbed frames -- so the forced slice-ring line is left out.
--look=1: the same frame in the NV20 look (option shadow_look 1: NV20 Phong, the light buffer's opacity with the ambient
floor .05) on the same three paths; --look=0, the default, is the R8k look."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    perturb = "--perturb" in sys.argv[1:]
    looks = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--look=")]
    if any(v not in ("0", "1") for v in looks):
        sys.exit("--look=0 (the R8k look) or --look=1 (the NV20 look)")
    look = int(looks[-1]) if looks else 0
    n = int(args[0]) if len(args) > 0 else 512
    lb = int(args[1]) if len(args) > 1 else 1024
    pkg = bench.load_package()
    r = pkg.Renderer(0)
    vghf, nrm = bench.make_volume(r, n)
    r.upload_volume_device(vghf.data_ptr(), (n, n, n), 3, 1, nrm.data_ptr())
    del vghf, nrm
    xform, _ = bench.configure(r, "cfg3", n, 1024, 512)
    xf = [float(v) for v in xform.T.reshape(-1)]
    if look:
        r.set_shading("nv20", (3.0, 4.0, -3.0), bench.EYE, bench.AT, xf, bench.INTENS, 0.05)
    else:
        r.set_shading("r8k", (3.0, 4.0, -3.0), bench.EYE, bench.AT, xf, bench.INTENS)
    r.set_shadow(1, lb, 0.5)
    if look:
        r.set_option("shadow_look", look)
        print("shadow_look %d: NV20 Phong, amb .05" % look, flush=True)
    forms = [("two marches, eye pass on the slice-ring kernel", 1, 2), ("two marches, eye pass on the gather kernel", 1, 1),
             ("a launch per slice", 0, 0), ("auto", 1, 0)]
    if perturb:
        r.set_option("shadow_perturb", 1)
        r.set_perturb(bench.libc_noise_tex(32), (.2, .1, 0, 0), (.2, 2.1, 4.5, 8.7))
        forms = forms[1:]
        print("perturbed fetch: weights (.2, .1), scales (.2, 2.1)", flush=True)
    frame = torch.zeros((1024 * 1024, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    keep = {}
    for name, march, kernel in forms:
        r.set_option("shadow_march", march)
        r.set_option("kernel", kernel)
        for _ in range(40 if kernel != 1 else 3):
            r.render_device(frame.data_ptr(), None, st)
        torch.cuda.synchronize()
        r.timing_reset()
        for _ in range(10):
            r.render_device(frame.data_ptr(), None, st)
        torch.cuda.synchronize()
        kms, _ = r.timing_read()
        keep[name] = (frame.clone(), torch.from_numpy(r.light_buffer()))
        kid = r.last_frame_info()[0]
        tile = " %dx%d px tiles, %d+%d waves" % tuple(int(r.stat("slab_plan_" + f)) for f in ("tw", "th", "nw", "nl")) if kid == 2 else ""
        print("%-48s %.3f ms per frame (kernel id %d%s)" % (name, kms, kid, tile), flush=True)
    names = list(keep)
    for n in names[1:]:
        print("%s vs %s: frames max |diff| %.3g, light buffers identical: %s" % (
            names[0], n, float((keep[names[0]][0] - keep[n][0]).abs().max()), bool((keep[names[0]][1] == keep[n][1]).all())), flush=True)
    print("max alpha %.3f" % float(keep[names[0]][0][:, 3].max()), flush=True)
    r.close()


if __name__ == "__main__":
    main()
