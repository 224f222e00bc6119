#!/usr/bin/env python3
"""Cost of stepping through a time series on the device-resident cache (developer tool, GPU box only).  Config 3's scene
(f32 VGH of the reference generator's spheres, 1024^2 x 512 planes), four steps = four seeds.
  1. a settled frame of one step, the first frame of a new pose, and select + the next frame for every switch;
  2. a playback loop over 4 cached steps, one frame per step: all four resident (capacity 4), then capacity 2 with
     each next step uploaded (smk_upload_timestep_device) on a second stream while the current one renders.
Frame times are HIP-event times on the render stream (median); the loop also reports wall time per frame.
    python tools/timestep_time.py [volume edge] [loop frames]
  3. --blend: fractional time (smk_blend_timesteps).  For f32, u8 and u16 steps: the blend alone and
     smk_upload_timestep_device of the same step alone (HIP events round the entry's work on its stream, median of 9), the
     bytes both move, and the blend's time against the upload's times the ratio of their bytes; then, for f32, playback
     over the four resident steps with 4 blended frames between neighbours, each blend enqueued on a second stream beside
     the frame before it.  Writes the note profiles/timestep_blend.md (--out PATH: elsewhere).
    python tools/timestep_time.py --blend [--out PATH] [volume edge] [loop frames]
  4. --download: reading a step back (smk_download_timestep_device).  For u8, u16 and f32 steps: the download alone and
     smk_upload_timestep_device of the same step alone (as in 3.), the bytes both move, their ratio; then, for f32, playback
     over the four resident steps with and without a download of the shown step on a second stream beside each frame.
     Writes the note profiles/step_download.md (--out PATH: elsewhere).
    python tools/timestep_time.py --download [--out PATH] [volume edge] [loop frames]
  5. --derive: derivatives of a step (smk_derive_timestep).  For u8, u16 and f32 rings: the blend and the derive of it (HIP
     events round the two entries' work on their stream, median of 9) against the seven-call recipe of INTEGRATION.md 5 in
     the same run -- blend, download, strided copy of channel 0, stream synchronise, smk_make_vgh_device,
     smk_normals_*_device, smk_upload_timestep_device --: its device work stage by stage and its wall time, host wait
     included; then, for f32, playback over the four resident steps with a blend and a derive on a second stream beside each
     frame.  Writes the note profiles/step_derive.md (--out PATH: elsewhere).
    python tools/timestep_time.py --derive [--out PATH] [volume edge] [loop frames]
  6. --merge: merged fields of a step (smk_merge_timestep).  The same two comparisons for a multi-field series -- config 3's
     step read as two fields and G --: the blend and the merge of it against the recipe -- blend, download, strided copy of
     the fields, stream synchronise, smk_merge_fields_device / smk_merge_fields_f32_device (for a u16 ring: the fields as
     floats, the float merge, smk_quantize_u16_device of G, the voxels put together), smk_upload_timestep_device --; then,
     for f32, playback with a blend and a merge on a second stream beside each frame.  Writes profiles/step_merge.md.
    python tools/timestep_time.py --merge [--out PATH] [volume edge] [loop frames]
  7. --shards: the stencil producers on a shard (smk_step_extremes_device + smk_derive_timestep_shard / smk_merge_timestep_shard).
     Rank 0 of an 8-way shard of a series of twice the edge (edge 512: a 1024^3 series, a stored box of about 512^3), halo 4:
     blend + export + write pass on one stream for u8, u16 and f32 rings, HIP events, no host wait (the rank's own words
     stand in for the combined ones: the device work is the same); beside it, in the same run, the unsharded one-call
     entries alone on a step of edge^3, `repeats` times over so that their run-to-run spread shows; the shard rank as a ratio
     to the unsharded entry per voxel written.  Replaces the section "## Times on one MI355X" of profiles/step_shard.md (what
     stands before it, the kernels' resource table, stays; --out PATH: another file, treated alike).
    python tools/timestep_time.py --shards [--out PATH] [volume edge] [repeats]
  8. --blocks: time steps from a rank's own dense block (smk_block_extremes_device + smk_upload_timestep_scalar_block_device /
     smk_upload_timestep_fields_block_device).  Rank 0 of an 8-way shard of a series of that edge, declared without data, halo
     4: the block route's export + write for u8, u16 and f32 rings, HIP events, `repeats` rounds after warm-up; in the same
     run the packed route, the only one before: smk_upload_timestep_device of the whole volume's interleaved array, then
     smk_step_extremes_device, then smk_*_timestep_shard.  Replaces the section "## Times on one MI355X" of
     profiles/step_block.md (what stands before it, the kernels' resource table, stays).
    python tools/timestep_time.py --blocks [--out PATH] [volume edge] [repeats]"""
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


def event_ms(stream, work):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    work()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def typed_steps(R, n, dtype):
    """four steps of config 3's volume on the device as (data, normals) tensors of that voxel type, and its smk_dtype"""
    out = []
    for seed in (1, 2, 3, 4):
        vghf, nrm = bench.make_volume(R, n, seed=seed)
        if dtype == "u8":
            data = (vghf * 255.0 + 0.5).to(torch.uint8)
        elif dtype == "u16":
            data = torch.empty(vghf.shape, dtype=torch.int16, device="cuda")     # (the bits of uint16 voxels)
            R.quantize_u16_device(vghf.data_ptr(), vghf.numel(), data.data_ptr())
        else:
            data = vghf
        out.append((data, nrm))
    torch.cuda.synchronize()
    return out, {"u8": 0, "f32": 1, "u16": 2}[dtype]


def kernel_registers():
    """{kernel: its entry} of the built library's kernels (tools/kernel_inventory.py), or {} where that fails"""
    import json
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "simian-spacemonkey_amd", "csrc", "libsmk_hip.so")
    try:
        with tempfile.TemporaryDirectory() as d:
            subprocess.run([sys.executable, os.path.join(root, "tools", "kernel_inventory.py"), lib, "-o", os.path.join(d, "k.json")],
                           check=True, capture_output=True, timeout=600)
            inv = json.load(open(os.path.join(d, "k.json")))
    except Exception:
        return {}
    return inv


def blend_leg(pkg, n, loop, out_path):
    lines = ["# Fractional time: `smk_blend_timesteps` on one MI355X", "",
             "Written by `tools/timestep_time.py --blend %d %d`.  Config 3's step (%d^3 VGH with normals), HIP-event times" % (n, loop, n),
             "round the entry's work on its stream (blend or pack, then the brick summaries), median of 9 after 3 warm-up calls.",
             "Bytes: the blend reads two stored volumes and writes one, and the summary reads the result (4 x stored); the upload",
             "reads the caller's voxels and normals, writes the stored volume, and the summary reads it.  The yardstick is the",
             "upload, the code that was there before: the blend should take no more than the ratio of the two kernels' bytes",
             "(3 x stored : source + stored; 3/2 for f32, 24/14 for u8) times the upload's time, with 20 % for run-to-run spread.", "",
             "| voxels | stored bytes | blend ms | blend TB/s | upload ms | upload TB/s | byte ratio | blend / upload | within ratio x 1.2 |",
             "|---|---|---|---|---|---|---|---|---|"]
    bl = torch.cuda.Stream()
    dims = (n, n, n)
    for dtype in ("f32", "u8", "u16"):
        R = pkg.Renderer(0)
        try:
            steps, dt = typed_steps(R, n, dtype)
            R.set_timestep_cache(6)
            R.upload_volume_device(steps[0][0].data_ptr(), dims, 3, dt, steps[0][1].data_ptr())
            for t in (1, 2, 3):
                R.upload_timestep_device(t, steps[t][0].data_ptr(), dims, 3, dt, steps[t][1].data_ptr(), stream=bl.cuda_stream)
            torch.cuda.synchronize()
            stored = n ** 3 * (16 if dtype == "f32" else 8)
            source = n ** 3 * (3 * {"f32": 4, "u8": 1, "u16": 2}[dtype] + 3)
            tb = [event_ms(bl, lambda i=i: R.blend_timesteps(0, 1, 0.3, 10 + (i & 1), stream=bl.cuda_stream)) for i in range(12)][3:]
            tu = [event_ms(bl, lambda: R.upload_timestep_device(3, steps[3][0].data_ptr(), dims, 3, dt, steps[3][1].data_ptr(),
                                                                stream=bl.cuda_stream)) for _ in range(12)][3:]
            b_ms, u_ms = statistics.median(tb), statistics.median(tu)
            ratio = 3.0 * stored / (source + stored)
            ok = b_ms <= ratio * u_ms * 1.2
            lines.append("| %s | %.0f MiB | %.3f (min %.3f, max %.3f) | %.2f | %.3f (min %.3f, max %.3f) | %.2f | %.3f | %.3f | %s |" % (
                dtype, stored / 2 ** 20, b_ms, min(tb), max(tb), 4.0 * stored / b_ms / 1e9, u_ms, min(tu), max(tu),
                (source + 2.0 * stored) / u_ms / 1e9, ratio, b_ms / u_ms, "yes" if ok else "NO"))
            print(lines[-1], flush=True)
            if dtype == "f32":
                play = blend_playback(R, n, loop, bl)
        finally:
            R.close()
            torch.cuda.synchronize()
    lines += ["", "## Playback", "", "Config 3's scene (f32, 1024^2 x 512 planes) over the four resident steps, every step followed by 4 blended frames",
              "(w = 0.2 .. 0.8) towards the next one; the blend of frame i + 1 is enqueued on a second stream before frame i, into the",
              "output id frame i does not show.  DESIGN.md 3b has 0.72 ms per frame for whole resident steps and 1.79 ms with the next",
              "step uploaded beside the frame.", ""] + play
    regs = {k: v for k, v in kernel_registers().items() if "smk_k_blend" in k}
    lines += ["", "## Kernels", "", "`smk_k_blend_steps<FORM>`: 256 lanes, 4 x 16-byte units of each source per lane and turn, loads before arithmetic, at most",
              "2048 workgroups striding over the box.  No scratch, no LDS.  FORM 0: bytes (u8 voxels, the separate normals buffer), 1: f32",
              "with the normal bytes in .w, 2: u16, 3: four-channel f32.  VGPRs from `tools/kernel_inventory.py`:", ""]
    lines += ["- `%s`: %d VGPRs, %d bytes of scratch" % (k, v["vgprs"], v["private_segment"]) for k, v in sorted(regs.items())] or ["- (inventory not available here)"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("wrote", out_path, flush=True)


def download_leg(pkg, n, loop, out_path):
    lines = ["# Reading a step back: `smk_download_timestep_device` on one MI355X", "",
             "Written by `tools/timestep_time.py --download %d %d`.  Config 3's step (%d^3, three channels with normals), HIP-event" % (n, loop, n),
             "times round the entry's work on its stream, median of 9 after 3 warm-up calls.  Bytes: the download reads the stored",
             "volume and writes the caller's voxels and normals (stored + source); the upload, the yardstick measured in the same",
             "run, reads the caller's arrays, writes the stored volume, and its brick summary reads that again (source + 2 x stored).",
             "Nothing is gated: the expectation is the upload's time times the ratio of the bytes.", "",
             "| voxels | stored | source | download ms | download TB/s | upload ms | upload TB/s | byte ratio | download / upload |",
             "|---|---|---|---|---|---|---|---|---|"]
    bl = torch.cuda.Stream()
    dims = (n, n, n)
    play = []
    for dtype in ("u8", "u16", "f32"):
        R = pkg.Renderer(0)
        try:
            steps, dt = typed_steps(R, n, dtype)
            R.set_timestep_cache(4)
            R.upload_volume_device(steps[0][0].data_ptr(), dims, 3, dt, steps[0][1].data_ptr())
            for t in (1, 2, 3):
                R.upload_timestep_device(t, steps[t][0].data_ptr(), dims, 3, dt, steps[t][1].data_ptr(), stream=bl.cuda_stream)
            torch.cuda.synchronize()
            esz = {"f32": 4, "u8": 1, "u16": 2}[dtype]
            stored = n ** 3 * (16 if dtype == "f32" else 8)
            source = n ** 3 * (3 * esz + 3)
            out_d = torch.zeros(n ** 3 * 3 * esz, dtype=torch.uint8, device="cuda")
            out_g = torch.zeros(n ** 3 * 3, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            td = [event_ms(bl, lambda: R.download_timestep_device(out_d.data_ptr(), out_g.data_ptr(), 1, bl.cuda_stream)) for _ in range(12)][3:]
            tu = [event_ms(bl, lambda: R.upload_timestep_device(3, steps[3][0].data_ptr(), dims, 3, dt, steps[3][1].data_ptr(),
                                                                stream=bl.cuda_stream)) for _ in range(12)][3:]
            # what came back is what went up (u16: the third channel to its stored 8 bits)
            src_d = steps[1][0].contiguous().view(torch.uint8).reshape(-1)
            if dtype == "u16":
                a16, b16 = out_d.view(torch.int16).view(-1, 3), steps[1][0].view(-1, 3)
                assert torch.equal(a16[:, :2], b16[:, :2]), "download differs from the uploaded step"
            else:
                assert torch.equal(out_d, src_d), "download differs from the uploaded step"
            assert torch.equal(out_g, steps[1][1].contiguous().view(torch.uint8).reshape(-1)), "normals differ from the uploaded step"
            d_ms, u_ms = statistics.median(td), statistics.median(tu)
            ratio = (stored + source) / (source + 2.0 * stored)
            lines.append("| %s | %.0f MiB | %.0f MiB | %.3f (min %.3f, max %.3f) | %.2f | %.3f (min %.3f, max %.3f) | %.2f | %.3f | %.3f |" % (
                dtype, stored / 2 ** 20, source / 2 ** 20, d_ms, min(td), max(td), (stored + source) / d_ms / 1e9, u_ms, min(tu), max(tu),
                (source + 2.0 * stored) / u_ms / 1e9, ratio, d_ms / u_ms))
            print(lines[-1], flush=True)
            if dtype == "f32":
                play = download_playback(R, n, loop, bl, out_d, out_g)
        finally:
            R.close()
            torch.cuda.synchronize()
    lines += ["", "## Playback", "", "Config 3's scene (f32, 1024^2 x 512 planes) over the four resident steps, one frame per step, first alone and then",
              "with a download of the shown step enqueued on a second stream beside each frame.", ""] + play
    regs = {k: v for k, v in kernel_registers().items() if "smk_k_unpack" in k}
    lines += ["", "## Kernels", "", "`smk_k_unpack_step<L>` (L 0: u8, 1: f32, 2: u16 voxels): 256 lanes, 4 x 16-byte units per lane and chunk, the next chunk's",
              "loads issued before this chunk's bytes are staged in LDS; whole 16-byte lines of the output go out as one store each, the",
              "ragged ends of a chunk's run byte by byte; at most 2048 workgroups striding over the chunks.  From `tools/kernel_inventory.py`:", ""]
    lines += ["- `%s`: %d VGPRs, %d bytes of scratch" % (k, v["vgprs"], v["private_segment"]) for k, v in sorted(regs.items())] or ["- (inventory not available here)"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("wrote", out_path, flush=True)


def wall_ms(work):
    t0 = time.perf_counter()
    work()
    return (time.perf_counter() - t0) * 1e3


def derive_leg(pkg, n, loop, out_path):
    lines = ["# Derivatives of a step: `smk_derive_timestep` on one MI355X", "",
             "Written by `tools/timestep_time.py --derive %d %d`.  Config 3's step (%d^3, three channels with normals); the source is" % (n, loop, n),
             "the 0.3 blend of two resident steps.  Median of 9 after 3 warm-up rounds.",
             "", "- **entry**: HIP events round `smk_blend_timesteps` + `smk_derive_timestep` on one stream (and round the derive alone):",
             "  seed, extremes pass, write pass, brick summaries.  No host wait.",
             "- **recipe** (INTEGRATION.md 5, the definition of the contract): blend, `smk_download_timestep_device`, a strided copy of",
             "  channel 0, a stream synchronise, `smk_make_vgh_device`, (`smk_quantize_u16_device` for a u16 ring,)",
             "  `smk_normals_*_device`, `smk_upload_timestep_device`.  Its device work is the sum of its stages: HIP events round the",
             "  asynchronous ones on their stream; the preparation entries run on the context's own stream and return when their",
             "  kernels are done, so their stage is the host time of the call on an idle device (it includes their launch, their",
             "  allocation and their device-to-host copy of the extremes, which are part of that path).  Wall: host time from the first",
             "  call to the end of a final synchronise, the host wait in the middle included.",
             "", "The condition of the feature: the entry's device time lies below the recipe's in the same run.", "",
             "| ring | derive alone ms | blend + derive ms | recipe device ms (blend+download+copy / make_vgh / quantise / normals / upload) | recipe wall ms | entry / recipe device | below |",
             "|---|---|---|---|---|---|---|"]
    bl = torch.cuda.Stream()
    dims = (n, n, n)
    nv = n ** 3
    play = []
    for dtype in ("u8", "u16", "f32"):
        R = pkg.Renderer(0)
        try:
            steps, dt = typed_steps(R, n, dtype)
            R.set_timestep_cache(8)
            R.upload_volume_device(steps[0][0].data_ptr(), dims, 3, dt, steps[0][1].data_ptr())
            for t in (1, 2, 3):
                R.upload_timestep_device(t, steps[t][0].data_ptr(), dims, 3, dt, steps[t][1].data_ptr(), stream=bl.cuda_stream)
            torch.cuda.synchronize()
            esz = {"f32": 4, "u8": 1, "u16": 2}[dtype]
            tdt = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.int16}[dtype]
            out_d = torch.zeros((nv, 3), dtype=tdt, device="cuda")       # the recipe's four scratch arrays (five for u16)
            s0 = torch.zeros(nv, dtype=tdt, device="cuda")
            vgh8 = torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            vghf = torch.zeros(nv * 3, dtype=torch.float32, device="cuda") if dtype != "u8" else None
            q16 = torch.zeros(nv * 3, dtype=torch.int16, device="cuda") if dtype == "u16" else None
            nrm = torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            sb = bl.cuda_stream
            t_derive, t_entry, t_recipe, t_wall = [], [], [], []
            for i in range(12):
                R.blend_timesteps(0, 1, 0.3, 10, stream=sb)
                t_derive.append(event_ms(bl, lambda: R.derive_timestep(10, 12, 1, 0, stream=sb)))
                t_entry.append(event_ms(bl, lambda: (R.blend_timesteps(0, 1, 0.3, 10, stream=sb), R.derive_timestep(10, 12, 1, 0, stream=sb))))
                torch.cuda.synchronize()
                w0 = time.perf_counter()

                def front():
                    R.blend_timesteps(0, 1, 0.3, 11, stream=sb)
                    R.download_timestep_device(out_d.data_ptr(), None, 11, sb)
                    with torch.cuda.stream(bl):
                        s0.copy_(out_d[:, 0])
                st_front = event_ms(bl, front)                           # (event_ms ends with the host wait of the recipe)
                st_vgh = wall_ms(lambda: R.make_vgh_device(s0.data_ptr(), dt, dims, 1, vgh8.data_ptr() if dtype == "u8" else None,
                                                           vghf.data_ptr() if vghf is not None else None))
                st_q = wall_ms(lambda: R.quantize_u16_device(vghf.data_ptr(), nv * 3, q16.data_ptr())) if dtype == "u16" else 0.0
                if dtype == "u8":
                    st_n = wall_ms(lambda: R.normals_vgh_device(vgh8.data_ptr(), 3, dims, 0, nrm.data_ptr()))
                else:
                    st_n = wall_ms(lambda: R.normals_f32_device(vghf.data_ptr(), 3, dims, 0, nrm.data_ptr()))
                up = vgh8 if dtype == "u8" else q16 if dtype == "u16" else vghf
                st_up = event_ms(bl, lambda: R.upload_timestep_device(13, up.data_ptr(), dims, 3, dt, nrm.data_ptr(), stream=sb))
                torch.cuda.synchronize()
                t_wall.append((time.perf_counter() - w0) * 1e3)
                t_recipe.append((st_front, st_vgh, st_q, st_n, st_up))
            # the two results are the same step
            a_d, a_g = torch.zeros_like(out_d), torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            b_d, b_g = torch.zeros_like(out_d), torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            R.blend_timesteps(0, 1, 0.3, 11, stream=sb)
            R.derive_timestep(11, 12, 1, 0, stream=sb)
            R.download_timestep_device(a_d.data_ptr(), a_g.data_ptr(), 12, sb)
            R.download_timestep_device(b_d.data_ptr(), b_g.data_ptr(), 13, sb)
            torch.cuda.synchronize()
            assert torch.equal(a_d.view(torch.uint8), b_d.view(torch.uint8)) and torch.equal(a_g, b_g), "the derive differs from the recipe"
            med = statistics.median
            d_ms, e_ms, w_ms = med(t_derive[3:]), med(t_entry[3:]), med(t_wall[3:])
            stages = [med([r[j] for r in t_recipe[3:]]) for j in range(5)]
            r_ms = sum(stages)
            lines.append("| %s | %.3f (min %.3f, max %.3f) | %.3f (min %.3f, max %.3f) | %.3f (%s) | %.3f | %.3f | %s |" % (
                dtype, d_ms, min(t_derive[3:]), max(t_derive[3:]), e_ms, min(t_entry[3:]), max(t_entry[3:]), r_ms,
                " / ".join("%.3f" % v for v in stages), w_ms, e_ms / r_ms, "yes" if e_ms < r_ms else "NO"))
            print(lines[-1], flush=True)
            if dtype == "f32":
                del out_d, s0, vgh8, vghf, nrm, a_d, a_g, b_d, b_g
                play = derive_playback(R, n, loop, bl)
        finally:
            R.close()
            torch.cuda.synchronize()
    lines += ["", "## Playback", "", "Config 3's scene (f32, 1024^2 x 512 planes) over the four resident steps, every step followed by 4 frames of",
              "fractional time (w = 0.2 .. 0.8) towards the next one, each showing the DERIVED step of its blend; blend and derive of",
              "frame i + 1 are enqueued on a second stream before frame i, into the output ids frame i does not show.", ""] + play
    regs = {k: v for k, v in kernel_registers().items() if "smk_k_derive" in k}
    lines += ["", "## Kernels", "", "`smk_k_derive_stats<SRC>` and `smk_k_derive_write<SRC, OUT>` (SRC 0..2: a dense u8 / f32 / u16 scalar, 3..5: channel 0 of",
              "packed u8 / u16 / f32 voxels; OUT: the ring's type): one workgroup of 256 lanes per 32 x 8 x 8 tile, the scalar as floats in",
              "LDS with a 2-voxel apron (20 736 bytes; the write pass keeps the scaled V beside it: 41 472 bytes), a lane per (x, y)",
              "column of 8 voxels, one 8- or 16-byte store per voxel.  From `tools/kernel_inventory.py`:", ""]
    fam = [(name, [v for k, v in regs.items() if name in k]) for name in ("smk_k_derive_seed", "smk_k_derive_stats", "smk_k_derive_write")]
    lines += ["- `%s`: %d instance%s, %d - %d VGPRs, at most %d bytes of scratch" % (
        name, len(vs), "" if len(vs) == 1 else "s", min(v["vgprs"] for v in vs), max(v["vgprs"] for v in vs),
        max(v["private_segment"] for v in vs)) for name, vs in fam if vs] or ["- (inventory not available here)"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("wrote", out_path, flush=True)


def merge_leg(pkg, n, loop, out_path):
    lines = ["# Merged fields of a step: `smk_merge_timestep` on one MI355X", "",
             "Written by `tools/timestep_time.py --merge %d %d`.  Config 3's step (%d^3, three channels with normals) read as a" % (n, loop, n),
             "multi-field step: two fields and G.  The source is the 0.3 blend of two resident steps.  Median of 9 after 3 warm-up rounds.",
             "", "- **entry**: HIP events round `smk_blend_timesteps` + `smk_merge_timestep` on one stream (and round the merge alone):",
             "  seed, maximum pass, write pass, brick summaries.  No host wait.  Bytes counted for the merge alone: the two passes read",
             "  the stored source, the write pass writes the stored output, the summaries read it: 4 x stored.",
             "- **recipe** (INTEGRATION.md 5, the definition of the contract): blend, `smk_download_timestep_device`, a strided copy of",
             "  the two fields, a stream synchronise, the merge entry (`smk_merge_fields_device` for u8, `smk_merge_fields_f32_device`",
             "  for f32; for a u16 ring the fields as floats, the float merge, `smk_quantize_u16_device` of G and the voxels put together),",
             "  `smk_upload_timestep_device`.  Its device work is the sum of its stages: HIP events round the asynchronous ones on",
             "  their stream; the merge and quantise entries run on the context's own stream and return when their kernels are done,",
             "  so their stage is the host time of the call on an idle device (it includes their launch and their allocation, which",
             "  are part of that path).  Wall: host time from the first call to the end of a final synchronise.",
             "", "The condition of the feature: the entry's device time does not exceed the recipe's in the same run, on any ring type.", "",
             "| ring | merge alone ms | merge GB/s | blend + merge ms | recipe device ms (blend+download+copy / merge / quantise+compose / upload) | recipe wall ms | entry / recipe device | not above |",
             "|---|---|---|---|---|---|---|---|"]
    bl = torch.cuda.Stream()
    dims = (n, n, n)
    nv = n ** 3
    play = []
    for dtype in ("u8", "u16", "f32"):
        R = pkg.Renderer(0)
        try:
            steps, dt = typed_steps(R, n, dtype)
            R.set_timestep_cache(8)
            R.upload_volume_device(steps[0][0].data_ptr(), dims, 3, dt, steps[0][1].data_ptr(), dmode="V2G")
            for t in (1, 2, 3):
                R.upload_timestep_device(t, steps[t][0].data_ptr(), dims, 3, dt, steps[t][1].data_ptr(), dmode="V2G", stream=bl.cuda_stream)
            torch.cuda.synchronize()
            tdt = {"f32": torch.float32, "u8": torch.uint8, "u16": torch.int16}[dtype]
            mdt = torch.uint8 if dtype == "u8" else torch.float32
            out_d = torch.zeros((nv, 3), dtype=tdt, device="cuda")       # the recipe's scratch arrays
            f2 = torch.zeros((nv, 2), dtype=mdt, device="cuda")
            mg = torch.zeros((nv, 3), dtype=mdt, device="cuda")
            g1 = torch.zeros(nv, dtype=torch.float32, device="cuda") if dtype == "u16" else None
            q1 = torch.zeros(nv, dtype=torch.int16, device="cuda") if dtype == "u16" else None
            v16 = torch.zeros((nv, 3), dtype=torch.int16, device="cuda") if dtype == "u16" else None
            nrm = torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            sb = bl.cuda_stream
            t_merge, t_entry, t_recipe, t_wall = [], [], [], []
            for i in range(12):
                R.blend_timesteps(0, 1, 0.3, 10, stream=sb)
                t_merge.append(event_ms(bl, lambda: R.merge_timestep(10, 12, stream=sb)))
                t_entry.append(event_ms(bl, lambda: (R.blend_timesteps(0, 1, 0.3, 10, stream=sb), R.merge_timestep(10, 12, stream=sb))))
                torch.cuda.synchronize()
                w0 = time.perf_counter()

                def front():
                    R.blend_timesteps(0, 1, 0.3, 11, stream=sb)
                    R.download_timestep_device(out_d.data_ptr(), None, 11, sb)
                    with torch.cuda.stream(bl):
                        if dtype == "u16":                               # F = (float)v of the 16-bit values, unscaled
                            f2.copy_(out_d[:, :2].to(torch.int32) & 0xffff)
                        else:
                            f2.copy_(out_d[:, :2])
                st_front = event_ms(bl, front)                           # (event_ms ends with the host wait of the recipe)
                if dtype == "u8":
                    st_m = wall_ms(lambda: R.merge_fields_device(f2.data_ptr(), 2, dims, mg.data_ptr(), nrm.data_ptr()))
                else:
                    st_m = wall_ms(lambda: R.merge_fields_f32_device(f2.data_ptr(), 2, dims, mg.data_ptr(), nrm.data_ptr()))
                st_q = 0.0
                if dtype == "u16":
                    def gcopy():
                        with torch.cuda.stream(bl):
                            g1.copy_(mg[:, 2])
                    st_q = event_ms(bl, gcopy)
                    st_q += wall_ms(lambda: R.quantize_u16_device(g1.data_ptr(), nv, q1.data_ptr()))

                    def compose():
                        with torch.cuda.stream(bl):
                            v16[:, :2].copy_(out_d[:, :2])
                            v16[:, 2].copy_(q1)
                    st_q += event_ms(bl, compose)
                up = v16 if dtype == "u16" else mg
                st_up = event_ms(bl, lambda: R.upload_timestep_device(13, up.data_ptr(), dims, 3, dt, nrm.data_ptr(), dmode="V2G", stream=sb))
                torch.cuda.synchronize()
                t_wall.append((time.perf_counter() - w0) * 1e3)
                t_recipe.append((st_front, st_m, st_q, st_up))
            # the two results are the same step
            a_d, a_g = torch.zeros_like(out_d), torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            b_d, b_g = torch.zeros_like(out_d), torch.zeros(nv * 3, dtype=torch.uint8, device="cuda")
            R.blend_timesteps(0, 1, 0.3, 11, stream=sb)
            R.merge_timestep(11, 12, stream=sb)
            R.download_timestep_device(a_d.data_ptr(), a_g.data_ptr(), 12, sb)
            R.download_timestep_device(b_d.data_ptr(), b_g.data_ptr(), 13, sb)
            torch.cuda.synchronize()
            assert torch.equal(a_d.view(torch.uint8), b_d.view(torch.uint8)) and torch.equal(a_g, b_g), "the merge differs from the recipe"
            med = statistics.median
            m_ms, e_ms, w_ms = med(t_merge[3:]), med(t_entry[3:]), med(t_wall[3:])
            stages = [med([r[j] for r in t_recipe[3:]]) for j in range(4)]
            r_ms = sum(stages)
            stored = nv * (16 if dtype == "f32" else 8)
            lines.append("| %s | %.3f (min %.3f, max %.3f) | %.0f | %.3f (min %.3f, max %.3f) | %.3f (%s) | %.3f | %.3f | %s |" % (
                dtype, m_ms, min(t_merge[3:]), max(t_merge[3:]), 4 * stored / m_ms / 1e6, e_ms, min(t_entry[3:]), max(t_entry[3:]), r_ms,
                " / ".join("%.3f" % v for v in stages), w_ms, e_ms / r_ms, "yes" if e_ms <= r_ms else "NO"))
            print(lines[-1], flush=True)
            if dtype == "f32":
                del out_d, f2, mg, nrm, a_d, a_g, b_d, b_g
                play = derive_playback(R, n, loop, bl, make=lambda src, out: R.merge_timestep(src, out, stream=bl.cuda_stream), what="merge")
        finally:
            R.close()
            torch.cuda.synchronize()
    lines += ["", "## Playback", "", "Config 3's scene (f32, 1024^2 x 512 planes) over the four resident steps, every step followed by 4 frames of",
              "fractional time (w = 0.2 .. 0.8) towards the next one, each showing the MERGED step of its blend; blend and merge of",
              "frame i + 1 are enqueued on a second stream before frame i, into the output ids frame i does not show.", ""] + play
    regs = {k: v for k, v in kernel_registers().items() if "smk_k_merge_seed" in k or "MergeParams" in k}
    lines += ["", "## Kernels", "", "`smk_k_merge_max<SRC, NF>` and `smk_k_merge_write<SRC, NF>` (SRC 0..2: dense u8 / f32 / u16 fields, 3..5: the channels of",
              "packed u8 / u16 / f32 voxels; NF: the number of fields): one workgroup of 256 lanes per tile of 64 units x 4 rows x 4 slices,",
              "a lane per 16-byte unit (two 8-byte voxels, or one f32 voxel) that marches through the tile's slices: the units before and",
              "behind stay in registers, the row's neighbours come from the neighbouring lanes, the units above and below are loaded",
              "straight through the caches; no LDS; one 16-byte store per unit.  From `tools/kernel_inventory.py`:", "",
              "| kernel | VGPRs | SGPRs | LDS bytes | scratch bytes |", "|---|---|---|---|---|"]
    lines += ["| `%s` | %d | %d | %d | %d |" % (k, v["vgprs"], v["sgprs"], v["group_segment"], v["private_segment"]) for k, v in sorted(regs.items())] \
        or ["| (inventory not available here) | | | | |"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("wrote", out_path, flush=True)


def derive_playback(R, n, loop, bl, make=None, what="derive"):
    frame = torch.zeros((SIZE * SIZE, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    bench.configure(R, "cfg3", n, SIZE, PLANES)
    for _ in range(24):
        timed_frame(R, frame, st)
    seq = [(t, (t + 1) % 4, j / 5.0) for t in range(4) for j in range(5)]

    def prepare(i, derive):    # what frame i shows: a whole step, or a blend (and its derived step) enqueued now
        a, b, w = seq[i % len(seq)]
        if w == 0:
            return a
        R.blend_timesteps(a, b, w, 10 + (i & 1), stream=bl.cuda_stream)
        if not derive:
            return 10 + (i & 1)
        if make:
            make(10 + (i & 1), 12 + (i & 1))
        else:
            R.derive_timestep(10 + (i & 1), 12 + (i & 1), 1, 0, stream=bl.cuda_stream)
        return 12 + (i & 1)
    out = []
    for label, derive in (("blends alone", False), ("a blend and a %s beside each fractional frame" % what, True)):
        for phase, frames in (("warm-up", len(seq)), ("timed", loop)):
            ev = []
            R.select_timestep(prepare(0, derive))
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for i in range(frames):
                nxt = prepare(i + 1, derive)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                R.render_device(frame.data_ptr(), None, st.cuda_stream)
                b.record(st)
                ev.append((a, b))
                R.select_timestep(nxt)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - w0) * 1e3 / frames
            ms = [a.elapsed_time(b) for a, b in ev]
            if phase == "timed":
                out.append("- %s: %d frames (4 of 5 fractional), frame median %.3f ms, max %.3f ms, wall %.3f ms per frame" % (
                    label, frames, statistics.median(ms), max(ms), wall))
                print(out[-1], flush=True)
    assert R.stat("slab_failures") == 0
    return out


def download_playback(R, n, loop, dl, out_d, out_g):
    frame = torch.zeros((SIZE * SIZE, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    bench.configure(R, "cfg3", n, SIZE, PLANES)
    for _ in range(24):
        timed_frame(R, frame, st)
    out = []
    for label, with_download in (("whole resident steps", False), ("with a download of the shown step beside each frame", True)):
        for phase, frames in (("warm-up", 8), ("timed", loop)):
            ev = []
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            cur = R.timesteps()[0]
            for _ in range(frames):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(st)
                R.render_device(frame.data_ptr(), None, st.cuda_stream)
                b.record(st)
                ev.append((a, b))
                if with_download:
                    R.download_timestep_device(out_d.data_ptr(), out_g.data_ptr(), stream=dl.cuda_stream)
                cur = (cur + 1) % 4
                R.select_timestep(cur)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - w0) * 1e3 / frames
            ms = [a.elapsed_time(b) for a, b in ev]
            if phase == "timed":
                out.append("- %s: %d frames, frame median %.3f ms, max %.3f ms, wall %.3f ms per frame" % (
                    label, frames, statistics.median(ms), max(ms), wall))
                print(out[-1], flush=True)
    assert R.stat("slab_failures") == 0
    return out


def blend_playback(R, n, loop, bl):
    frame = torch.zeros((SIZE * SIZE, 4), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    bench.configure(R, "cfg3", n, SIZE, PLANES)
    for _ in range(24):
        timed_frame(R, frame, st)
    seq = [(t, (t + 1) % 4, j / 5.0) for t in range(4) for j in range(5)]

    def prepare(i):    # what frame i shows: a whole step, or a blend enqueued now into the output the frame before does not read
        a, b, w = seq[i % len(seq)]
        if w == 0:
            return a
        R.blend_timesteps(a, b, w, 10 + (i & 1), stream=bl.cuda_stream)
        return 10 + (i & 1)
    out = []
    for label, frames in (("warm-up", len(seq)), ("timed", loop)):
        ev = []
        R.select_timestep(prepare(0))
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for i in range(frames):
            nxt = prepare(i + 1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            R.render_device(frame.data_ptr(), None, st.cuda_stream)
            b.record(st)
            ev.append((a, b))
            R.select_timestep(nxt)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) * 1e3 / frames
        ms = [a.elapsed_time(b) for a, b in ev]
        if label == "timed":
            out.append("- %d frames (4 of 5 blended): frame median %.3f ms, max %.3f ms, wall %.3f ms per frame, %d blends" % (
                frames, statistics.median(ms), max(ms), wall, int(R.stat("tblend_count"))))
            print(out[-1], flush=True)
    assert R.stat("slab_failures") == 0
    return out


def alone_ms(R, kind, stream, rounds=12, warm=3):
    """the one-call entry alone on the blend 10 of a context's steps 0 and 1: (median, min, max) ms of HIP events"""
    sb = stream.cuda_stream
    t = []
    for i in range(rounds):
        R.blend_timesteps(0, 1, 0.3, 10, stream=sb)
        if kind == "derive":
            t.append(event_ms(stream, lambda: R.derive_timestep(10, 12, 1, 0, stream=sb)))
        else:
            t.append(event_ms(stream, lambda: R.merge_timestep(10, 12, stream=sb)))
    t = t[warm:]
    return statistics.median(t), min(t), max(t)


def shards_leg(pkg, n, repeats, out_path):
    N, halo = 2 * n, 4
    lines = ["## Times on one MI355X", "",
             "Written by `tools/timestep_time.py --shards %d %d`.  Rank 0 of an 8-way shard of a %d^3 series (three channels with" % (n, repeats, N),
             "normals, halo %d: a stored box of %d^3 voxels of 8 bytes, %d^3 of f32) against an unsharded context that holds a %d^3" % (
                 halo, n + halo + (n + halo) % 2, n + halo, n),
             "step.  HIP events on one stream, median of 9 after 3 warm-up rounds (min - max); the source is the 0.3 blend of two resident",
             "steps.  The shard's write pass reads the rank's own exported words: the combine is a host's 8-word MAX all-reduce and no",
             "device work.  *Per voxel written*: (export + write) / stored voxels over the one-call entry / its stored voxels.", "",
             "| ring | entry | shard: blend + export + write ms | export ms | write ms | unsharded one-call entry alone ms, %d repeats (median, min - max) | shard / unsharded per voxel written |" % repeats,
             "|---|---|---|---|---|---|---|"]
    st = torch.cuda.Stream()
    sb = st.cuda_stream
    med = statistics.median
    for dtype in ("u8", "u16", "f32"):
        # the unsharded yardstick first: edge^3
        R = pkg.Renderer(0)
        un = {}
        try:
            steps, dt = typed_steps(R, n, dtype)
            R.set_timestep_cache(8)
            R.upload_volume_device(steps[0][0].data_ptr(), (n, n, n), 3, dt, steps[0][1].data_ptr())
            R.upload_timestep_device(1, steps[1][0].data_ptr(), (n, n, n), 3, dt, steps[1][1].data_ptr(), stream=sb)
            torch.cuda.synchronize()
            del steps
            for kind in ("derive", "merge"):
                un[kind] = [alone_ms(R, kind, st) for _ in range(repeats)]
            unvox = (n + (n % 2 if dtype != "f32" else 0)) ** 2 * n     # the stored box of the unsharded step
        finally:
            R.close()
            torch.cuda.synchronize()
        dt = {"u8": 0, "f32": 1, "u16": 2}[dtype]            # smk_dtype
        R = pkg.Renderer(0)
        try:
            R.set_shard(0, 8)
            R.set_option("halo", halo)
            R.set_timestep_cache(6)
            for t in (0, 1):                                 # one step of the series at a time is on the device beside the ring
                vghf, nrm = bench.make_volume(R, N, seed=t + 1)
                if dtype == "u8":
                    data = (vghf * 255.0 + 0.5).to(torch.uint8)
                elif dtype == "u16":
                    data = torch.empty(vghf.shape, dtype=torch.int16, device="cuda")
                    R.quantize_u16_device(vghf.data_ptr(), vghf.numel(), data.data_ptr())
                else:
                    data = vghf
                torch.cuda.synchronize()
                if t == 0:
                    R.upload_volume_device(data.data_ptr(), (N, N, N), 3, dt, nrm.data_ptr())
                else:
                    R.upload_timestep_device(1, data.data_ptr(), (N, N, N), 3, dt, nrm.data_ptr(), stream=sb)
                torch.cuda.synchronize()
                del vghf, nrm, data
                torch.cuda.empty_cache()
            edge = n + halo + ((n + halo) % 2 if dtype != "f32" else 0)
            shvox = edge * edge * (n + halo)
            words = torch.zeros(8, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            wp = words.data_ptr()
            for kind, code in (("derive", 0), ("merge", 1)):
                def write():
                    if kind == "derive":
                        R.derive_timestep_shard(10, 12, wp, 1, 0, stream=sb)
                    else:
                        R.merge_timestep_shard(10, 12, wp, stream=sb)
                t_all, t_ex, t_wr = [], [], []
                for i in range(12):
                    t_all.append(event_ms(st, lambda: (R.blend_timesteps(0, 1, 0.3, 10, stream=sb), R.step_extremes_device(code, 10, wp, stream=sb), write())))
                    t_ex.append(event_ms(st, lambda: R.step_extremes_device(code, 10, wp, stream=sb)))
                    t_wr.append(event_ms(st, write))
                assert R.timestep_halo(12) == halo - (2 if kind == "derive" else 1)
                a, e, w = t_all[3:], t_ex[3:], t_wr[3:]
                u = un[kind]
                umed = med([x[0] for x in u])
                ratio = ((med(e) + med(w)) / shvox) / (umed / unvox)
                lines.append("| %s | %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %s | %.2f |" % (
                    dtype, kind, med(a), min(a), max(a), med(e), min(e), max(e), med(w), min(w), max(w),
                    "; ".join("%.3f (%.3f - %.3f)" % x for x in u), ratio))
                print(lines[-1], flush=True)
        finally:
            R.close()
            torch.cuda.synchronize()
    # the section replaces the one the file has; what stands before it stays
    head = open(out_path).read() if os.path.exists(out_path) else ""
    if lines[0] in head:
        head = head[:head.index(lines[0])]
    if head and not head.endswith("\n\n"):
        head = head.rstrip("\n") + "\n\n"
    open(out_path, "w").write(head + "\n".join(lines) + "\n")
    print("wrote", out_path, flush=True)


def blocks_leg(pkg, n, repeats, out_path):
    """rank 0 of an 8-way shard of an n^3 series: the block route against the packed route, per ring and producer"""
    halo, warm = 4, 3
    e = n // 2 + halo                                        # rank 0's block: its region and `halo` ghost cells, from voxel 0
    lines = ["## Times on one MI355X", "",
             "Written by `tools/timestep_time.py --blocks %d %d`.  Rank 0 of an 8-way shard of a %d^3 series (three channels, no" % (n, repeats, n),
             "normals, halo %d), declared with `smk_declare_volume`; the rank's block is its region plus %d ghost cells, %d^3 elements" % (halo, halo, e),
             "from voxel 0.  HIP events on one stream, median of %d after %d warm-up rounds (min - max).  *Block route*:" % (repeats, warm),
             "`smk_block_extremes_device` + the block write pass, straight from the dense arrays.  *Packed route*, the only one before",
             "the block entries: `smk_upload_timestep_device` of the WHOLE volume's interleaved `(s, 0, 0)` or `(f0, f1, 0)` array (which",
             "a rank of a decomposed simulation does not hold), then `smk_step_extremes_device`, then `smk_*_timestep_shard`.  Both write",
             "passes read the rank's own exported words: the combine is a host's 8-word MAX all-reduce and no device work.", "",
             "| ring | entry | block route ms | its export ms | its write ms | packed route ms | its pack ms | its export ms | its write ms | block / packed |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    st = torch.cuda.Stream()
    sb = st.cuda_stream
    med = statistics.median
    tdt = {"u8": torch.uint8, "u16": torch.int16, "f32": torch.float32}
    for dtype in ("u8", "u16", "f32"):
        dt = {"u8": 0, "f32": 1, "u16": 2}[dtype]
        R = pkg.Renderer(0)
        try:
            R.set_shard(0, 8)
            R.set_option("halo", halo)
            R.set_timestep_cache(4)
            R.declare_volume((n, n, n), 3, dt, normals=False)
            g = torch.Generator(device="cuda").manual_seed(7)
            whole = torch.zeros((n, n, n, 3), dtype=tdt[dtype], device="cuda")       # the packed route's array: the whole volume
            for ch in (0, 1):
                f = torch.rand((n, n, n), generator=g, device="cuda")
                whole[..., ch] = f if dtype == "f32" else (f * (255 if dtype == "u8" else 32767)).to(tdt[dtype])
            del f
            fields = [whole[:e, :e, :e, ch].contiguous() for ch in (0, 1)]           # the block route's: the rank's own dense arrays
            blk = pkg.smk_block((0, 0, 0), (e, e, e))
            words = torch.zeros(8, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            wp = words.data_ptr()
            for kind, code in (("derive", 0), ("merge", 1)):
                ptrs = [f.data_ptr() for f in (fields[:1] if kind == "derive" else fields)]
                if kind == "derive":
                    whole[..., 1] = 0                        # (s, 0, 0); the second field comes back for the merge below
                    torch.cuda.synchronize()

                def bex():
                    R.block_extremes_device(code, ptrs, dt, blk, wp, stream=sb)

                def bwr():
                    if kind == "derive":
                        R.upload_timestep_scalar_block_device(12, ptrs[0], dt, blk, wp, 1, 0, stream=sb)
                    else:
                        R.upload_timestep_fields_block_device(12, ptrs, dt, blk, wp, stream=sb)

                def pack():
                    R.upload_timestep_device(10, whole.data_ptr(), (n, n, n), 3, dt, None, stream=sb)

                def pex():
                    R.step_extremes_device(code, 10, wp, stream=sb)

                def pwr():
                    if kind == "derive":
                        R.derive_timestep_shard(10, 13, wp, 1, 0, stream=sb)
                    else:
                        R.merge_timestep_shard(10, 13, wp, stream=sb)
                t = {k: [] for k in ("b", "bex", "bwr", "p", "pack", "pex", "pwr")}
                for i in range(warm + repeats):
                    t["b"].append(event_ms(st, lambda: (bex(), bwr())))
                    t["p"].append(event_ms(st, lambda: (pack(), pex(), pwr())))
                    for k, f in (("bex", bex), ("bwr", bwr), ("pack", pack), ("pex", pex), ("pwr", pwr)):
                        t[k].append(event_ms(st, f))
                assert R.timestep_halo(12) == R.timestep_halo(13) == halo - (2 if kind == "derive" else 1)
                t = {k: v[warm:] for k, v in t.items()}
                lines.append("| %s | %s | %s | %.2f |" % (dtype, kind, " | ".join(
                    "%.3f (%.3f - %.3f)" % (med(t[k]), min(t[k]), max(t[k])) for k in ("b", "bex", "bwr", "p", "pack", "pex", "pwr")),
                    med(t["b"]) / med(t["p"])))
                print(lines[-1], flush=True)
                if kind == "derive":                         # the second field again, for the merge
                    whole[:e, :e, :e, 1] = fields[1]
                    torch.cuda.synchronize()
        finally:
            R.close()
            del whole, fields
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
    head = open(out_path).read() if os.path.exists(out_path) else ""
    if lines[0] in head:
        head = head[:head.index(lines[0])]
    if head and not head.endswith("\n\n"):
        head = head.rstrip("\n") + "\n\n"
    open(out_path, "w").write(head + "\n".join(lines) + "\n")
    print("wrote", out_path, flush=True)


def main():
    args = sys.argv[1:]
    blend, download, derive, merge = "--blend" in args, "--download" in args, "--derive" in args, "--merge" in args
    shards, blocks = "--shards" in args, "--blocks" in args
    out_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                            "step_block.md" if blocks else "step_shard.md" if shards else "step_merge.md" if merge else "step_derive.md" if derive else "step_download.md" if download else "timestep_blend.md")
    if "--out" in args:
        out_path = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    args = [a for a in args if a not in ("--blend", "--download", "--derive", "--merge", "--shards", "--blocks")]
    n = int(args[0]) if len(args) > 0 else 512
    loop = int(args[1]) if len(args) > 1 else 32
    pkg = bench.load_package()
    if blocks:
        return blocks_leg(pkg, n, int(args[1]) if len(args) > 1 else 5, out_path)
    if shards:
        return shards_leg(pkg, n, int(args[1]) if len(args) > 1 else 3, out_path)
    if merge:
        return merge_leg(pkg, n, loop, out_path)
    if derive:
        return derive_leg(pkg, n, loop, out_path)
    if download:
        return download_leg(pkg, n, loop, out_path)
    if blend:
        return blend_leg(pkg, n, loop, out_path)
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
