"""Half-angle shadows on sharded contexts (smk.h "Shadows on shards"): P shard contexts on one GPU run phase 1,
the light exchange and their frames; merged in smk_shard_order's order, the frame equals the unsharded frame with shadows
(itself pinned to the CPU checker by tests/test_gpu_shadow.py) within a few ulp.  Also: the ranks' eye and light samples
partition the unsharded frame's exactly, every rank's light history agrees with the unsharded one wherever its eye pass
can look, the slice set is the whole volume's on every rank, and what cannot be composed is refused."""
import numpy as np
import pytest

from _scenes import make_scene, push_scene

pytestmark = pytest.mark.gpu
TOL = 2e-5

LIGHTS = {"eye_side": (0, 0, -5), "oblique": (3, 4, -3), "behind": (-2, 3, 4), "side": (5, 1, 0.5), "low": (-4, -2, -3)}

# (ranks, kind, f32, shade, pose, light, extra): u8 and f32, 2-D and 3-D tables, no and R8k shading, both slice directions
# and lights on both sides of every split plane (tests/test_shadow_shards_cpu.py checks that the list covers them), a clip
# plane, a ragged volume whose midpoints split unevenly
CASES = [
    (2, "cfg3", False, 1, "rot", "oblique", None),
    (2, "cfg3", True, 0, "back", "behind", None),
    (4, "cfg3", True, 1, "rot", "low", None),
    (4, "tf3d", False, 0, "rot", "side", None),
    (4, "cfg3", False, 1, "rot", "oblique", "clip"),
    (8, "cfg3", True, 1, "rot", "eye_side", None),
    (8, "tf3d", False, 1, "back", "oblique", None),
    (8, "cfg3", False, 0, "side", "side", None),
    (8, "cfg3", True, 1, "rot", "oblique", "ragged"),
    (2, "cfg2", False, 0, "rot", "side", "cplane"),
]


def case_scene(kind, f32, shade, pose, light, extra):
    sc = make_scene(kind, f32=f32, shade=shade, pose=pose, dims=(45, 38, 41) if extra == "ragged" else None)
    sc.light_pos = LIGHTS[light]
    sc.shadow = (64, 0.75)
    if extra == "clip":
        sc.clip = (3, tuple(0.55 * float(f) for f in sc.fsize))      # Y+: what lies below y = .55 stays
    if extra == "cplane":
        sc.clip_plane = (0.3, -0.2, 0.93, 6.9)
    return sc


def _whole(factory, sc):
    R = factory()
    push_scene(R, sc)
    return R


def _shards(factory, sc, world, halo=None):
    """P shard contexts; each with the halo its frame with shadows needs (smk_get_shadow_margin) unless given"""
    rs = []
    try:
        for r in range(world):
            R = factory()
            R.set_shard(r, world)
            if halo is not None:
                R.set_option("halo", halo)
            push_scene(R, sc)
            if halo is None:
                need = R.shadow_margin()[1]
                R.close()
                R = factory()
                R.set_shard(r, world)
                R.set_option("halo", need)
                push_scene(R, sc)
            rs.append(R)
    except Exception:
        for R in rs:
            R.close()
        raise
    return rs


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(x) for x in c if x is not None) for c in CASES])
def test_sharded_shadow_frame_equals_whole(gpu_renderer_factory, smk, case):
    from simian_spacemonkey_amd import sortlast
    world = case[0]
    sc = case_scene(*case[1:])
    W = _whole(gpu_renderer_factory, sc)
    rs = []
    try:
        ref = W.render()
        assert ref[..., 3].max() > 0.05 and W.light_buffer()[..., 3].max() > 0.05, "vacuous scene"
        rs = _shards(gpu_renderer_factory, sc, world)
        got = sortlast.render_shadow_frame_local(rs).cpu().numpy()
        for R in rs:
            assert R.stat("slab_status") == 0
        err = float(np.abs(got - ref).max())
        assert err <= TOL, f"merged sharded frame vs unsharded: max abs err {err}"
    finally:
        W.close()
        for R in rs:
            R.close()


def _texel_samples(c, k):
    """voxel position of every light-buffer texel's slice-k sample, float64 [LB][LB][3] (the light march's placement)"""
    x = np.arange(c.LB, dtype=np.float64) + 0.5
    a = x * c.las + c.lal
    A, B = np.meshgrid(a, a)                     # [y][x]
    G = np.stack([A * c.Gx[q] + B * c.Gy[q] + c.Gc[q] for q in range(3)], -1)
    nG = A * c.nGx + B * c.nGy + c.nGc
    w = (k * c.ldnum + c.lnum0) / nG
    return np.asarray(c.Lc, np.float64) + w[..., None] * G


@pytest.mark.parametrize("world", [2, 4, 8])
def test_partition_coefficients_and_light_histories(gpu_renderer_factory, smk, world):
    from simian_spacemonkey_amd import sortlast
    sc = case_scene("cfg3", world != 4, 1, "rot", "oblique" if world != 8 else "low", None)
    W = _whole(gpu_renderer_factory, sc)
    rs = []
    try:
        W.render()
        coef = W.shadowcoef()
        fields = [f for f, _ in coef._fields_]

        def val(c, f):
            v = getattr(c, f)
            return list(v) if hasattr(v, "__len__") else v
        rs = _shards(gpu_renderer_factory, sc, world)
        # the slice set and the light projection are the whole volume's on every rank, bit for bit
        for R in rs:
            c = R.shadowcoef()
            assert [val(c, f) for f in fields] == [val(coef, f) for f in fields]
        # every eye sample and every light sample of the unsharded frame belongs to exactly one rank
        assert sum(R.count_samples() for R in rs) == W.count_samples()
        assert sum(R.stat("light_samples") for R in rs) == W.stat("light_samples")
        assert W.stat("light_samples") > 0
        sortlast.render_shadow_frame_local(rs)
        # rank j's history (E_j over H_j) == the unsharded one at the texels whose slice-k sample lies in grown(j)
        n = coef.nslices
        checked = 0
        for k in sorted({n // 4, n // 2, (3 * n) // 4, n - 1, n}):
            whole = W.light_history(k)
            pos = _texel_samples(coef, k)
            for j, R in enumerate(rs):
                m = R.shadow_margin()[0]
                g0, g1 = sortlast.shard_region(sc.dims, j, world)
                inside = np.ones(pos.shape[:2], bool)
                for a in range(3):
                    inside &= (pos[..., a] >= g0[a] - 0.5 - m + 0.01) & (pos[..., a] <= g1[a] - 0.5 + m - 0.01)
                if not inside.any():
                    continue
                got = R.light_history(k)
                err = float(np.abs(got[inside] - whole[inside]).max())
                assert err <= TOL, f"rank {j} slice {k}: light history max abs err {err}"
                checked += int((whole[inside][:, 3] > 0).sum())
        assert checked > 0, "no non-empty texel compared"
    finally:
        W.close()
        for R in rs:
            R.close()


def test_the_host_driven_exchange_equals_the_in_process_one(gpu_renderer_factory, smk):
    """steps 1-2 by hand (smk_shadow_exports_device, an all-to-all of the slots, smk_shadow_entries_device) == the same
    frame with smk_shadow_exchange_local, bit for bit; and the light order is the BSP order from the light rays' apex"""
    import torch
    from simian_spacemonkey_amd import sortlast
    world = 4
    sc = case_scene("cfg3", False, 1, "rot", "low", None)
    rs = _shards(gpu_renderer_factory, sc, world)
    try:
        a = sortlast.render_shadow_frame_local(rs).cpu().numpy()
        c = rs[0].shadowcoef()
        lb = c.LB
        exports = torch.zeros((world, world, lb, lb, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for r, R in enumerate(rs):
            R.shadow_exports_device(exports[r].data_ptr())
        torch.cuda.synchronize()
        assert float(exports[0, 0].abs().max()) == 0.0            # slot r of rank r: zero
        entries = exports.transpose(0, 1).contiguous()             # entries[j][r] = exports[r][j]
        for j, R in enumerate(rs):
            R.shadow_entries_device(entries[j].data_ptr())
        torch.cuda.synchronize()
        npix = sc.width * sc.height
        layers = torch.zeros((world, npix, 4), dtype=torch.float32, device="cuda")
        for r, R in enumerate(rs):
            R.render_device(layers[r].data_ptr())
        torch.cuda.synchronize()
        out = torch.zeros((npix, 4), dtype=torch.float32, device="cuda")
        rs[0].composite_over_device(layers.data_ptr(), world, rs[0].shard_order(world), npix, out.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(a.shape), a)
        # the entries matter: the same frame with zero entries (every rank's light from its own samples only) differs
        zeros = torch.zeros_like(entries)
        torch.cuda.synchronize()
        for j, R in enumerate(rs):
            R.shadow_entries_device(zeros[j].data_ptr())
            R.render_device(layers[j].data_ptr())
        torch.cuda.synchronize()
        rs[0].composite_over_device(layers.data_ptr(), world, rs[0].shard_order(world), npix, out.data_ptr())
        torch.cuda.synchronize()
        assert float(np.abs(out.cpu().numpy().reshape(a.shape) - a).max()) > 1e-3
        assert rs[0].shard_light_order(world) == sortlast.front_to_back_order(list(c.Lc), sc.dims, world)
    finally:
        for R in rs:
            R.close()


def test_refusals_and_no_leak(gpu_renderer_factory, smk):
    import torch
    sc = case_scene("cfg3", False, 1, "rot", "oblique", None)
    rs = _shards(gpu_renderer_factory, sc, 2)
    plain = make_scene("cfg3", shade=1)
    try:
        R = rs[0]
        # no entries since the last frame
        with pytest.raises(smk.SmkError, match="whole volume on one GPU.*smk_shadow_entries_device"):
            R.render()
        lb = R.shadowcoef().LB
        zeros = torch.zeros((2, lb, lb, 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        # entries are consumed by a frame: a second frame without new ones fails again
        R.shadow_entries_device(zeros.data_ptr())
        R.render()
        with pytest.raises(smk.SmkError, match="whole volume on one GPU"):
            R.render()
        # the per-slice path stays single-GPU
        R.set_option("shadow_march", 0)
        R.shadow_entries_device(zeros.data_ptr())
        with pytest.raises(smk.SmkError, match="whole volume on one GPU.*shadow_march 0"):
            R.render()
        R.set_option("shadow_march", 1)
        # too small a halo: the message names the halo needed
        need = R.shadow_margin()[1]
        assert need >= 2
        thin = gpu_renderer_factory()
        rs.append(thin)
        thin.set_shard(1, 2)
        push_scene(thin, sc)                      # default halo 1
        thin.shadow_entries_device(zeros.data_ptr())
        with pytest.raises(smk.SmkError, match="halo >= %d" % thin.shadow_margin()[1]):
            thin.render()
        # nothing leaks into the next plain frame: bit-identical to a fresh context's
        for X in (R, thin):
            push_scene(X, plain, upload=False)
            got = X.render()
            F = gpu_renderer_factory()
            try:
                F.set_shard(0 if X is R else 1, 2)
                if X is R:
                    F.set_option("halo", need)
                push_scene(F, plain)
                assert np.array_equal(got, F.render())
            finally:
                F.close()
    finally:
        for R in rs:
            R.close()
