"""What the slice-ring kernel's loaders rely on, proved for every pitch the window-pitch rule can emit
(tests/_slab_plan_ref.py: the rule as DESIGN.md section 4 states it).  No GPU."""
import numpy as np

import _slab_plan_ref as ref

# the pitch classes DESIGN.md names: multiples of 8 units, and 12, 20, 28
NAMED = {8: (1, 8), 12: (3, 16), 16: (1, 4), 20: (5, 16), 24: (3, 8), 28: (7, 16), 32: (1, 2), 40: (5, 8), 48: (3, 4),
         56: (7, 8), 64: (1, 1)}
# ... and the one it does not name but the rule emits: a window of at most 4 units (an f32 volume 2-4 voxels across the
# view, a u8 one up to 8) that is more than 8 rows high.  Its next multiple of 4 is 4, with per = 4 / gcd(64, 4) = 1 -- a
# period the loaders know -- and 16 rows to the chunk instead of the 8 of pitch 8: fewer chunks, so the rule (and the
# planner, which the GPU sweep reads back) takes it.  The lane cover below holds for it like for any other pitch.
UNNAMED = {4: (1, 16)}


def test_reachable_pitch_classes():
    got = ref.emitted_pitches()
    classes = {wp: (per, rpg) for (wp, per, rpg) in got}
    assert len(classes) == len(got), "a pitch with two periods: %r" % sorted(got)
    want = dict(NAMED)
    want.update(UNNAMED)
    assert classes == want, "the rule emits %r" % sorted(classes.items())
    # pitch 4 needs a narrow AND tall window; every window wider than 4 units gets a named pitch
    for (wp, per, rpg), (wu, wv) in got.items():
        if wp == 4:
            assert wu <= 4 and wv > 8
    assert all(ref.pitch(wu, wv) in NAMED for wu in range(5, 65) for wv in range(1, 300))
    assert all(ref.pitch(wu, wv) == 8 for wu in range(1, 5) for wv in range(1, 9))
    assert all(per in ref.LOADER_PERIODS for per, _ in classes.values())


def test_lane_cover_of_every_emitted_pitch():
    """lanes 0..63 of chunks k = 0..per-1 at (row, col) = divmod(64 k + lane, wp) cover an rpg x wp block exactly once"""
    for (wp, per, rpg) in ref.emitted_pitches():
        assert 64 * per == rpg * wp, (wp, per, rpg)
        assert per <= 7                                  # the loader keeps voff[7], rowk[7], colk[7]
        unit = 64 * np.arange(per)[:, None] + np.arange(64)[None, :]
        row, col = np.divmod(unit, wp)
        hits = np.zeros((rpg, wp), int)
        assert row.max() == rpg - 1 and col.max() == wp - 1
        np.add.at(hits, (row, col), 1)
        assert (hits == 1).all(), (wp, per, rpg)
        # every chunk has a lane in column 0 (the loader's per-chunk column masks are never empty)
        assert ((col == 0).any(axis=1)).all(), wp
        # ... and the image of group g + 1 starts per * 1024 bytes behind that of group g: the flat image continues
        assert (unit.reshape(-1) == row.reshape(-1) * wp + col.reshape(-1)).all()


def test_the_rule_takes_the_cheaper_pitch_only():
    """DESIGN.md's own example, and the rule's two conditions at their edges"""
    assert ref.plan(17, 32, True, 64) == dict(wp=20, per=5, rpg=16, groups=2, chunks=10, wv=32)
    assert ref._cost(24, 32) == 12
    # a tie keeps the multiple of 8 (17 units x 16 rows: 5 chunks on 20, 6 on 24; x 8 rows: 5 against 3)
    assert ref.pitch(17, 8) == 24 and ref.pitch(17, 16) == 20
    # pitches whose period the loaders do not know are never taken, however tall the window
    for wu, by4 in ((33, 36), (41, 44), (49, 52), (57, 60)):
        assert ref._lattice(by4)[0] > 7
        assert all(ref.pitch(wu, wv) == by4 + 4 for wv in range(1, 200))
    # small workgroups: whole groups where the stored box has the rows, else the rows as sized
    assert ref.plan(17, 17, False, 64) == dict(wp=24, per=3, rpg=8, groups=3, chunks=9, wv=24)
    assert ref.plan(17, 17, False, 23)["wv"] == 17 and ref.plan(17, 17, True, 64)["wv"] == 17
    for wu in range(1, 65):
        for wv in (1, 7, 8, 9, 16, 17, 33, 100):
            for big in (False, True):
                p = ref.plan(wu, wv, big, 40)
                assert p["wp"] >= wu and p["wp"] - wu < 8 and p["groups"] * p["rpg"] >= p["wv"] >= wv
                assert p["chunks"] == p["groups"] * p["per"] <= ref._cost(-(-wu // 8) * 8, wv)
                ok, _ = ref.check_readback(wu, p["wv"], big, 40, p)
                assert ok
