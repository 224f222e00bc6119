"""The present rule itself (include/smk.h "display-ready frames"), pinned on the numpy restatement the GPU tests compare the
kernel with (tests/_present_ref.py): the quantiser's edges, the background blend, the window depth and its inverse."""
import numpy as np

import _present_ref as PR

F = np.float32


def test_quantiser_edges():
    q = PR.quantise
    assert q(F(0)) == 0 and q(F(1)) == 255 and q(F(0.5)) == 128
    k = np.arange(256)
    assert np.array_equal(q((k.astype(F) / F(255)).astype(F)), k.astype(np.uint8))
    for v in (np.nan, -0.0, -1.0, -np.inf, 1e-45, -1e-45, 1e-39, 1.1754942e-38):
        assert q(F(v)) == 0, v
    for v in (1.5, np.inf, 1.0000001):
        assert q(F(v)) == 255, v
    # round half up at the bin edges: (k + .5) / 255 is where k becomes k + 1
    assert q(F(0.49) / F(255)) == 0 and q(F(0.51) / F(255)) == 1
    assert q(F(254.49) / F(255)) == 254 and q(F(254.51) / F(255)) == 255
    # monotone over a dense sweep
    x = np.linspace(-0.25, 1.25, 200001).astype(F)
    assert np.all(np.diff(q(x).astype(np.int32)) >= 0)


def test_background_blend():
    white = (1.0, 1.0, 1.0)
    assert PR.present_rgba8(np.zeros((1, 4), F), white).tolist() == [[255, 255, 255, 255]]
    # an opaque pixel hides the background; alpha is 255 whatever the frame's
    px = np.array([[0.25, 0.5, 0.75, 1.0]], F)
    assert PR.present_rgba8(px, white).tolist() == [[64, 128, 191, 255]]
    # half-covered over (0.2, 0.5, 0.9): C + (1 - A) b, fp32 op by op
    px = np.array([[0.1, 0.2, 0.3, 0.5]], F)
    want = [int(np.floor(F(F(F(c) + F(F(0.5) * F(b))) * F(255)) + F(0.5))) for c, b in zip((0.1, 0.2, 0.3), (0.2, 0.5, 0.9))]
    assert PR.present_rgba8(px, (0.2, 0.5, 0.9)).tolist() == [want + [255]]
    # NaN anywhere in the pixel's blend quantises to 0, never to garbage
    px = np.array([[0.1, np.nan, 0.3, np.nan]], F)
    assert PR.present_rgba8(px, white).tolist() == [[0, 0, 0, 255]]


def test_no_background_passes_alpha_through_q():
    rng = np.random.default_rng(3)
    fr = rng.uniform(-0.25, 1.25, (64, 4)).astype(F)
    out = PR.present_rgba8(fr, None)
    assert out.dtype == np.uint8 and np.array_equal(out[:, 3], PR.quantise(fr[:, 3]))
    assert np.array_equal(out[:, :3], PR.quantise(fr[:, :3]))
    assert PR.present_rgba8(np.array([[0, 0, 0, 0.5]], F)).tolist() == [[0, 0, 0, 128]]


def test_window_depth_edges_and_monotony():
    n, f = 1.0, 20.0
    zw = PR.window_depth
    assert zw(F(n), n, f) == 0.0 and zw(F(f), n, f) == 1.0
    assert zw(F(np.inf), n, f) == 1.0 and zw(F(np.nan), n, f) == 1.0
    for d in (0.5, 0.0, -3.0, -np.inf):
        assert zw(F(d), n, f) == 0.0, d
    assert zw(F(25.0), n, f) == 1.0                      # beyond the far plane: clamped
    assert zw(np.zeros(3, F), n, f).dtype == np.float32
    d = np.sort(np.random.default_rng(5).uniform(0.5, 22.0, 20000).astype(F))
    z = zw(d, n, f)
    assert np.all(np.diff(z) >= 0) and z.min() == 0.0 and z.max() == 1.0
    # glFrustum's mapping at mid range: z_ndc = (f + n) / (f - n) - 2 f n / ((f - n) d), z_w = (z_ndc + 1) / 2
    dd = 7.0
    assert abs(float(zw(F(dd), n, f)) - ((f + n) / (f - n) - 2 * f * n / ((f - n) * dd) + 1) / 2) < 1e-7


def test_window_depth_round_trip_through_the_occlusion_inverse():
    """d -> z_w (float64 here: the rule before its final rounding) -> INTEGRATION's inverse d = f n / (f - z_w (f - n))"""
    for n, f in ((1.0, 20.0), (0.1, 100.0), (2.5, 7.0)):
        d = np.random.default_rng(7).uniform(n, f, 5000).astype(F)
        d = d[(d > F(n)) & (d < F(f))]
        d64 = d.astype(np.float64)
        n64, f64 = np.float64(F(n)), np.float64(F(f))
        zw64 = (f64 * (d64 - n64)) / ((f64 - n64) * d64)
        back = PR.view_depth(zw64, n, f)
        assert (np.abs(back - d64) / d64).max() <= 1e-6
        # the float32 result is that value rounded once
        assert np.array_equal(PR.window_depth(d, n, f), zw64.astype(F))
    # ... and through the float32 the host gets, at the test scenes' clip planes: half an ulp of z_w below 1 is 2^-25, which
    # the inverse magnifies by d (f - n) / (f n) <= 19 in relative terms -- 5.7e-7
    n, f = 1.0, 20.0
    d = np.random.default_rng(8).uniform(n, f, 5000).astype(F)
    d = d[(d > F(n)) & (d < F(f))]
    back = PR.view_depth(PR.window_depth(d, n, f), n, f)
    assert (np.abs(back - d.astype(np.float64)) / d).max() <= 1e-6
