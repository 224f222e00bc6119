#!/usr/bin/env python3
"""Developer tool (GPU box): re-run chosen cases of the random-frame fuzz with the slice-ring plan printed.
    SMK_DEBUG=1 python tools/fuzz_one.py SEED CASE [CASE ...]
    python tools/fuzz_one.py --features SEED CASE [CASE ...]     cases of the feature fuzz (tests/_fuzz_features.py) through
                                                                  its three legs: the feature record, each leg's outcome and,
                                                                  per kernel, the worst pixel against the CPU checker"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import test_gpu_fuzz as F  # noqa: E402
from _scenes import push_scene  # noqa: E402
import bench  # noqa: E402


def worst_pixel(name, img, ref):
    d = np.abs(img - ref)
    j, i = np.unravel_index(d.max(axis=2).argmax(), d.shape[:2])
    print("   %s vs CPU: max %g at pixel (%d,%d): gpu %s cpu %s" % (name, d.max(), i, j, img[j, i], ref[j, i]), flush=True)


def features(pkg, seed, cases):
    import test_gpu_fuzz_features as FF
    R0 = pkg.Renderer(0)
    try:
        for case in cases:
            sc, ft, ref, rd = FF.case_of(seed, case)
            print("== " + FF.F.describe(ft), flush=True)
            print("   " + ", ".join("%s %s" % (k, ft[k]) for k in ("vol_seed", "rot", "eye", "trans", "frustum", "pert_w", "h_slider")))
            key = (seed, case)
            with FF.context_for(R0, pkg.Renderer, ft) as R:
                legs = (("gather", lambda: FF.leg_gather(R, key, sc, ft, ref, rd, pkg.SmkError, "  ")),
                        ("slice-ring", lambda: FF.leg_slice_ring(R, key, sc, ft, ref, pkg.SmkError, "  ")),
                        ("column-stream", lambda: FF.leg_column_stream(R, key, sc, ft, ref, pkg.SmkError, "  ", again=True)))
                for name, leg in legs:
                    try:
                        print("   %s -> %s" % (name, leg()), flush=True)
                    except AssertionError as e:
                        print("   %s FAILED %s" % (name, str(e)[-300:]), flush=True)
                FF.push(R, sc, ft, upload=False)
                for k, name in ((1, "gather"), (2, "slice-ring"), (3, "column-stream")):
                    img, why = FF.forced(R, k, pkg.SmkError)
                    if why is None:
                        worst_pixel(name, img, ref)
                    else:
                        print("   %s: not applicable: %s" % (name, why))
    finally:
        R0.close()


def main():
    pkg = bench.load_package()
    if sys.argv[1] == "--features":
        return features(pkg, int(sys.argv[2]), [int(a) for a in sys.argv[3:]])
    seed = int(sys.argv[1])
    want = set(int(a) for a in sys.argv[2:])
    R = pkg.Renderer(0)
    rng = np.random.default_rng(seed)
    for case in range(max(want) + 1):
        sc, kind, f32, dims = F.random_scene(rng)
        if case not in want:
            continue
        print("== case %d: %s dims %s f32 %d %dx%d x%d shade %d" % (case, kind, dims, f32, sc.width, sc.height, sc.steps, sc.shade_mode), flush=True)
        r = R
        if sc.shard:
            from simian_spacemonkey_amd import sortlast
            r = pkg.Renderer(0)
            r.set_shard(*sc.shard)
            sc.region = sortlast.shard_region(sc.dims, *sc.shard)
        print("   rate %.3f eye %s trans %s frustum %s shard %s clip %s region %s" % (sc.sample_rate, sc.eye, sc.trans, sc.frustum, sc.shard, sc.clip, sc.region))
        try:
            print("   ->", F.one_case(r, sc, ""), flush=True)
        except Exception as e:
            print("   FAILED " + str(e)[-300:], flush=True)
        ref = sc.render()
        for k in (1, 2):
            r.set_option("kernel", k)
            try:
                img = r.render()
                worst_pixel("kernel %d" % k, img, ref)
            except Exception as e:
                print("   kernel %d: %s" % (k, str(e)[-200:]))
        r.set_option("kernel", 0)
        if r is not R:
            r.close()
    R.close()


if __name__ == "__main__":
    main()
