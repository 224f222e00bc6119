"""The float64 checker of the clip-plane widget's data slice (tests/_clip_slice_ref.py) against what can be known without a
GPU: its coverage equals the GL slice pipeline's rasteriser for the same quad and camera, its pass rule is the reference's
twelve-row table, a plane outside the volume draws nothing (except on X-, which the reference does not test), and both
looks give hand-computed colours on a 4^3 volume.  Also the condition the GPU tests rely on: for their poses the coverage
decided in float32 differs from float64 on at most 0.1 % of the covered pixels."""
import numpy as np
import pytest

import gl_slices
import oracle as O
import _clip_slice_ref as CS
from _clip_slice_cases import AXES, CASE_POSE, GPU_QUADS, PASS_TABLE, POSES, SIZE, clip_vpos, widget_corners

FS = (1.0, 0.75, 0.5)
FRUSTUM = (-0.5 / 7, 0.5 / 7, -0.5 / 7, 0.5 / 7)
ZNEAR, ZFAR = 1.0, 20.0


def _mv(pose, fsize=FS):
    return O.modelview((0, 0, -7), (0, 0, 0), (0, 1, 0), (0, 0, 0), O.rotation(*POSES[pose]), fsize)


@pytest.mark.parametrize("pose", ["rot", "side"])
@pytest.mark.parametrize("oaxis", [1, 4, 5])
def test_coverage_equals_the_gl_rasteriser(oaxis, pose):
    size = 40
    mv = _mv(pose)
    quad = CS.moved_quad(widget_corners(oaxis, clip_vpos(oaxis, FS), FS), FS, oaxis)
    cover, _, _ = CS.intersect(quad, mv, FRUSTUM, ZNEAR, size, size)
    img = np.zeros((size, size, 4))
    # render_quad_slice issues its vertices 1, 0, 2, 3: handed (1, 0, 2, 3) it draws GL_QUADS (0, 1, 2, 3)
    edge = gl_slices.render_quad_slice(img, np.ones((4, 4, 4)), FS, mv, FRUSTUM, ZNEAR, ZFAR, quad[[1, 0, 2, 3]], 1.0)
    assert cover.sum() > 50, "vacuous"
    assert np.array_equal(cover[~edge], img[..., 3][~edge] > 0)
    assert edge.sum() < cover.sum()


@pytest.mark.parametrize("oaxis", sorted(AXES))
def test_pass_table(oaxis):
    c = widget_corners(oaxis, clip_vpos(oaxis, FS), FS)
    neg, pos = PASS_TABLE[oaxis]
    assert CS.pass_rule(oaxis, -0.5, c, FS) == neg
    assert CS.pass_rule(oaxis, 0.5, c, FS) == pos
    assert CS.pass_rule(oaxis, 0.0, c, FS) == 0
    # shadows: a before pass is dropped when the slices run away from the viewer, an after pass never
    for dv, p in ((-0.5, neg), (0.5, pos)):
        assert CS.pass_rule(oaxis, dv, c, FS, vdl=0.3) == (0 if p == 1 else 2)
        assert CS.pass_rule(oaxis, dv, c, FS, vdl=-0.3) == p
        assert CS.pass_rule(oaxis, dv, c, FS, vdl=0.0) == p


@pytest.mark.parametrize("frac", [-0.2, 0.0, 1.0, 1.3])
@pytest.mark.parametrize("oaxis", sorted(AXES))
def test_plane_outside_the_volume_draws_nothing_except_on_x_minus(oaxis, frac):
    c = widget_corners(oaxis, clip_vpos(oaxis, FS, frac), FS)
    for dv in (-0.5, 0.5):
        p = CS.pass_rule(oaxis, dv, c, FS)
        if oaxis == 2:
            assert p == (1 if dv > 0 else 2)      # no range test (R8kVolRen3D.cpp:835)
        else:
            assert p == 0


def _vol4():
    """4^3 voxels, 4 channels, constant along x and y: channel k of layer z is (10 + 60 z + 5 k)"""
    d = np.zeros((4, 4, 4, 4), np.uint8)
    for z in range(4):
        for k in range(4):
            d[z, :, :, k] = 10 + 60 * z + 5 * k
    return d


def test_colour_known_answers():
    """a Z+ plane at z = 0.5 fSize - 0.001 + 0.001 (the offset) = texture coordinate r = 0.5: halfway between layers 1 and
    2, so every channel is (layer 1 + layer 2) / 2 = (70 + 5 k + 130 + 5 k) / 2 = 100 + 5 k, / 255"""
    d = _vol4()
    fs = (1.0, 1.0, 1.0)
    size = 16
    mv = O.modelview((0, 0, -7), (0, 0, 0), (0, 1, 0), (0, 0, 0), O.rotation((1, 0, 0), 20), fs)
    vpos = (0.5, 0.5, float(np.float32(0.5) - np.float32(0.001)))
    corners = widget_corners(5, vpos, fs)
    alpha = 0.6
    c = [(100 + 5 * k) / 255.0 for k in range(4)]
    want = {
        ("r8k", "VGH"): [c[0] * alpha, c[1] * alpha, c[2] * alpha, alpha],          # four-byte texture, third axis: rgb
        ("r8k", "VGH_VG"): [c[0] * alpha, c[1] * alpha, c[0] * alpha, alpha],       # (L, L, L, A), green <- alpha
        ("r8k", "VGH_V"): [0.0, c[0] * alpha, 0.0, alpha],                          # (0, 0, 0, A), green <- alpha
        ("nv20", "VGH"): [c[0] * alpha, c[0] * alpha, c[0] * alpha, alpha],         # value * alpha, alpha
    }
    for (look, dmode), w in want.items():
        S, cover, depth = CS.slice_layer(d, dmode, fs, mv, FRUSTUM, ZNEAR, size, size, corners, 5, alpha, look)
        assert cover.sum() > 20
        assert np.abs(S[cover] - np.array(w)).max() < 2e-6, (look, dmode)    # (the float32 offset: r = 0.5 to 1e-7)
        assert np.all(S[~cover] == 0)
    # alpha beyond 1: the R8k shader saturates it (:3229-3232); a three-element volume gets texture alpha 50, which no
    # third-axis colour reads
    S, cover, _ = CS.slice_layer(d[..., :3], "VGH", fs, mv, FRUSTUM, ZNEAR, size, size, corners, 5, 1.7, "r8k")
    assert np.abs(S[cover] - np.array([c[0], c[1], c[2], 1.0])).max() < 2e-6
    # composition: before = V + (1 - V.a) S, after = S + (1 - S.a) V, GL_MAX before = max
    V = np.zeros((size, size, 4)) + np.array([.2, .1, .05, .5])
    S, cover, _ = CS.slice_layer(d, "VGH", fs, mv, FRUSTUM, ZNEAR, size, size, corners, 5, alpha, "r8k")
    s = np.array(want[("r8k", "VGH")])
    assert np.abs(CS.compose(V, S, cover, 1)[cover] - (V[0, 0] + .5 * s)).max() < 2e-6
    assert np.abs(CS.compose(V, S, cover, 2)[cover] - (s + (1 - alpha) * V[0, 0])).max() < 2e-6
    assert np.abs(CS.compose(V, S, cover, 1, blend_max=True)[cover] - np.maximum(V[0, 0], s)).max() < 2e-6
    assert np.array_equal(CS.compose(V, S, cover, 0), V)
    assert np.array_equal(CS.compose(V, S, cover, 2)[~cover], V[~cover])


def test_depth_is_the_view_depth():
    """the hit point taken through the modelview has -z = the reported depth"""
    mv = _mv("rot")
    quad = CS.moved_quad(widget_corners(1, clip_vpos(1, FS), FS), FS, 1)
    cover, hit, depth = CS.intersect(quad, mv, FRUSTUM, ZNEAR, 32, 32)
    M = np.array(mv).reshape(4, 4).T
    z = hit[cover] @ M[2, :3] + M[2, 3]
    assert np.abs(-z - depth[cover]).max() < 1e-12
    assert np.abs(hit[cover][:, 0] - quad[0, 0]).max() < 1e-12


@pytest.mark.parametrize("oaxis,frac,margin", GPU_QUADS)
def test_poses_do_not_hinge_on_float32_edges(oaxis, frac, margin):
    """the GPU tests leave out pixels within 1e-3 px of a projected edge and require them to be <= 0.1 % of the covered
    ones; their quads (GPU_QUADS under CASE_POSE at SIZE) are chosen so that already float32 against float64 coverage
    stays under that"""
    fs = (1.0, 1.0, 1.0)
    mv = _mv(CASE_POSE[oaxis], fs)
    quad = CS.moved_quad(widget_corners(oaxis, clip_vpos(oaxis, fs, frac), fs, margin), fs, oaxis)
    c64, _, _ = CS.intersect(quad, mv, FRUSTUM, ZNEAR, SIZE, SIZE)
    c32, _, _ = CS.intersect(quad, mv, FRUSTUM, ZNEAR, SIZE, SIZE, dtype=np.float32)
    edge = CS.edge_pixels(quad, mv, FRUSTUM, ZNEAR, ZFAR, SIZE, SIZE)
    assert c64.sum() > 300, "vacuous"
    assert (c64 != c32).sum() <= 1e-3 * c64.sum()
    assert edge.sum() <= 1e-3 * c64.sum()
