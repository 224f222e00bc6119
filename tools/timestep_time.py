#!/usr/bin/env python3
"""Cost of stepping through a time series on the device-resident cache (developer tool, GPU box only).  Config 3's scene
(f32 VGH of the reference generator's spheres, 1024^2 x 512 planes), four steps = four seeds.
  1. a settled frame of one step, the first frame of a new pose, and select + the next frame for every switch;
  2. a playback loop over 4 cached steps, one frame per step: all four resident (capacity 4), then capacity 2 with
     each next step uploaded (smk_upload_timestep_device) on a second stream while the current one renders.
Frame times are HIP-event times on the render stream (median); the loop also reports wall time per frame.
    python tools/timestep_time.py [volume edge] [loop frames]"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

SIZE, PLANES = 1024, 512


def timed_frame(R, frame, st):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(st)
    R.render_device(frame.data_ptr(), None, st.cuda_stream)
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    loop = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    pkg = bench.load_package()
    frame = torch.zeros((SIZE * SIZE, 4), dtype=torch.float32, device="cuda")
    st, up = torch.cuda.Stream(), torch.cuda.Stream()
    R = pkg.Renderer(0)
    try:
        steps = [bench.make_volume(R, n, seed=s) for s in (1, 2, 3, 4)]
        torch.cuda.synchronize()
        dims = (n, n, n)
        R.set_timestep_cache(4)
        R.upload_volume_device(steps[0][0].data_ptr(), dims, 3, 1, steps[0][1].data_ptr())
        for t in (1, 2, 3):
            R.upload_timestep_device(t, steps[t][0].data_ptr(), dims, 3, 1, steps[t][1].data_ptr(), stream=st.cuda_stream)
        xform, mv = bench.configure(R, "cfg3", n, SIZE, PLANES)
        for _ in range(24):   # (auto mode's trials, the planner's measured weights)
            timed_frame(R, frame, st)
        settled = statistics.median(timed_frame(R, frame, st) for _ in range(9))
        print("step 0 settled frame: %.3f ms (median of 9)" % settled, flush=True)
        # the first frame of a new pose (camera turned by 2 degrees), then back
        turned = bench.rotation((1, 1, 0), 32)
        R.set_camera(bench.modelview(turned, (1.0, 1.0, 1.0)), bench.FRUSTUM, (1.0, 20.0), SIZE, SIZE)
        print("first frame of a new pose: %.3f ms" % timed_frame(R, frame, st), flush=True)
        R.set_camera(mv, bench.FRUSTUM, (1.0, 20.0), SIZE, SIZE)
        for _ in range(12):
            timed_frame(R, frame, st)
        for t in (1, 2, 3, 0, 2):
            h0 = time.perf_counter()
            R.select_timestep(t)
            hs = (time.perf_counter() - h0) * 1e3
            f1 = timed_frame(R, frame, st)
            f2 = timed_frame(R, frame, st)
            rest = statistics.median(timed_frame(R, frame, st) for _ in range(5))
            print("select %d: host %.3f ms, next frame %.3f ms, second %.3f ms, settled %.3f ms" % (t, hs, f1, f2, rest), flush=True)
        assert R.stat("slab_failures") == 0

        def playback(label, upload_next):
            ev = []
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            cur = R.timesteps()[0]
            for f in range(loop):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                R.render_device(frame.data_ptr(), None, st.cuda_stream)
                b.record(st)
                ev.append((a, b))
                nxt = (cur + 1) % 4
                if upload_next:   # the next step goes up on the second stream while this frame renders
                    R.upload_timestep_device(nxt, steps[nxt][0].data_ptr(), dims, 3, 1, steps[nxt][1].data_ptr(),
                                             stream=up.cuda_stream)
                R.select_timestep(nxt)
                cur = nxt
            torch.cuda.synchronize()
            wall = (time.perf_counter() - w0) * 1e3 / loop
            ms = [a.elapsed_time(b) for a, b in ev]
            print("%s: %d frames, frame median %.3f ms, max %.3f ms, wall %.3f ms per frame" % (
                label, loop, statistics.median(ms), max(ms), wall), flush=True)
        playback("playback, 4 steps resident", False)
        R.set_timestep_cache(2)
        playback("playback, capacity 2, next step uploaded on a second stream", True)
        assert R.stat("slab_failures") == 0
    finally:
        R.close()
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
