"""tests/_tf_correction.py, the numpy restatement of the 2-D table's opacity correction, against the CPU checker's
copyScale (byte for byte: 0 of 514 304 bytes differed over 2 009 rates when the bound was chosen, so it is equality),
known answers, and the steps-mode rate of a few checker scenes."""
import numpy as np
import pytest

import _tf_correction as T
from _scenes import make_scene

RATES = (0.4, 0.6, 0.75, 1.0, 1.5, 1.7, 2.5, 4.09375, 7.3)


def _ramp():
    tex = np.zeros((1, 256, 4), np.uint8)
    tex[0, :, 3] = np.arange(256)
    tex[0, :, :3] = 77
    return tex


def test_alpha_map_equals_the_checkers_copy_scale(O):
    ramp = _ramp()
    rng = np.random.default_rng(20)
    rates = [np.float32(r) for r in RATES] + list(rng.uniform(0.2, 9.0, 500).astype(np.float32))
    for sr in rates:
        want = O.copy_scale(ramp, float(sr))
        assert np.array_equal(T.alpha_map(sr), want[0, :, 3]), sr
        assert np.array_equal(T.apply(ramp, sr), want), sr


def test_known_answers():
    assert list(T.alpha_map(2.5)[[1, 2, 3, 128, 254, 255]]) == [0, 0, 1, 62, 227, 255]
    assert int(np.flatnonzero(T.alpha_map(7.3))[0]) == 8
    assert int(np.flatnonzero(T.alpha_map(2.5))[0]) == 3
    for sr in (0.4, 0.6, 0.75, 0.99):      # below 1 no visible texel becomes invisible
        assert T.alpha_map(sr)[1:].min() >= 1
    one = T.alpha_map(1.0).astype(int) - np.arange(256)       # rate 1: the identity up to the truncation of (1 - (1 - a/255)) * 255
    assert one.min() == -1 and one.max() == 0


def test_apply_touches_alpha_only():
    raw = T.ramp_table(100, 37)
    eff = T.apply(raw, 2.5)
    assert np.array_equal(eff[..., :3], raw[..., :3])
    assert np.array_equal(eff[..., 3], T.alpha_map(2.5)[raw[..., 3]])
    assert raw[..., 3].max() == 255          # (the input is not modified)


def test_ramp_table_uses_every_alpha_byte_and_has_its_bands():
    raw = T.ramp_table(256, 256)
    assert set(np.unique(raw[..., 3])) == set(range(256))
    lo, hi = T.low_band(256), T.high_band(256)
    assert lo[1] - lo[0] >= 8 and set(np.unique(raw[:, lo[0]:lo[1], 3])) == {1, 2}
    assert (raw[:, hi[0]:hi[1], 3] == 255).all()
    assert np.array_equal(raw, T.ramp_table(256, 256))          # seeded
    for sv, sg in ((64, 64), (100, 37), (33, 2), (2, 1)):
        t = T.ramp_table(sv, sg)
        assert t.shape == (sg, sv, 4) and t[..., 3].max() >= 175
        assert sv < 16 or (t[..., 3].max() == 255 and ((t[..., 3] > 0) & (t[..., 3] < 3)).any())


@pytest.mark.parametrize("pose,steps,dims,want", [
    ("id", 24, None, 0.75), ("id", 48, None, 1.5), ("id", 131, None, 4.09375), ("rot", 48, None, 0.9535117),
    ("id", 48, (40, 24, 18), 2.6666667)])
def test_steps_mode_rate(O, pose, steps, dims, want):
    sc = make_scene("cfg3", n=32, size=48, steps=steps, pose=pose, dims=dims)
    got = T.frame_rate(sc, 1.0, 1)
    assert got.dtype == np.float32 and got == np.float32(want), (got, want)
    assert T.frame_rate(sc, 2.0, 1) == np.float32(want) / np.float32(2.0)
    assert T.frame_rate(sc, 0.5, 0) == np.float32(2.0)


def test_sample_rate_mode_rate(O):
    sc = make_scene("cfg3", n=32, size=48, pose="rot")
    sc.steps, sc.sample_rate = 0, 2.5
    assert T.frame_rate(sc, 2.2, 1) == np.float32(2.5) / np.float32(2.2)
    assert T.frame_rate(sc, 2.2, 0) == np.float32(1) / np.float32(2.2)
