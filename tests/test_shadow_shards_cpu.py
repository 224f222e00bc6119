"""The frame cases of tests/test_gpu_shadow_shards.py cover what they claim to (CPU: the checker's shadow set-up)."""
from test_gpu_shadow_shards import CASES, case_scene


def test_cases_cover_both_slice_directions_and_both_sides_of_every_split(O):
    directions = set()
    sides = {0: set(), 1: set(), 2: set()}
    for case in CASES:
        world = case[0]
        sc = case_scene(*case[1:])
        c = sc.shadowcoef()
        directions.add(int(c.front_to_back))
        for bit in range(world.bit_length() - 1):          # bit 0 splits x, bit 1 y, bit 2 z
            a = bit % 3
            sides[a].add(c.Lc[a] >= sc.dims[a] // 2 - 0.5)
    assert directions == {0, 1}
    for a in range(3):
        assert sides[a] == {False, True}, "axis %d: the light apex on one side of the split only" % a
