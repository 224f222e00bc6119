"""The slice-ring kernel's window-pitch rule, restated from DESIGN.md section 4 ("The LDS image of a window is flat on a
pitch ...") -- not from the planner's code -- so that the sweep of tests/test_gpu_slab_plans.py can hold the planner's
read-back against a second opinion, and tests/test_slab_plan_ref.py can prove what the loaders rely on.

The rule.  A window row is `wu` 16-byte units, the LDS image of a slice is flat, and one DMA wave-instruction ("chunk")
writes 64 consecutive units of it.  On a pitch of `wp` units the (row, column) that lane l of chunk k serves is
divmod(64 k + l, wp); it repeats after lcm(64, wp) units = `per` chunks = `rpg` rows (a "group").  A slice of `wv` rows is
ceil(wv / rpg) groups of per chunks each.
  * the pitch is the next multiple of 8 units at or above wu;
  * or the next multiple of 4, where that is another number, its period is one the loaders know (per <= 7) and the slice
    then takes fewer chunks;
  * small workgroups load whole groups: wv is rounded up to groups * rpg where the stored box (Dv rows) has that many.
"""
from math import gcd

LOADER_PERIODS = (1, 3, 5, 7)     # the chunk counts per group the loader's code is written out for
MAX_UNITS = 64                    # a window row is at most one chunk


def _lattice(wp):
    """(per, rpg) of a pitch: lcm(64, wp) units are per chunks of 64 and rpg rows of wp"""
    span = 64 * wp // gcd(64, wp)
    return span // 64, span // wp


def _cost(wp, wv):
    per, rpg = _lattice(wp)
    return -(-wv // rpg) * per


def pitch(wu, wv):
    """the pitch the rule gives a window of wu units x wv rows"""
    assert 1 <= wu <= MAX_UNITS and wv >= 1
    by8 = -(-wu // 8) * 8
    by4 = -(-wu // 4) * 4
    if by4 != by8 and _lattice(by4)[0] <= max(LOADER_PERIODS) and _cost(by4, wv) < _cost(by8, wv):
        return by4
    return by8


def plan(wu, wv, big, Dv):
    """dict(wp, per, rpg, groups, chunks, wv) for a window of wu units x wv rows (wv as sized from the view, before the
    small workgroups' rounding) over a stored box of Dv rows"""
    wp = pitch(wu, wv)
    per, rpg = _lattice(wp)
    groups = -(-wv // rpg)
    if not big and groups * rpg <= Dv:
        wv = groups * rpg
    return dict(wp=wp, per=per, rpg=rpg, groups=groups, chunks=groups * per, wv=wv)


def check_readback(wu, wv, big, Dv, got):
    """The planner's read-back (wp, per, rpg, groups, chunks of a launch whose window is wu x wv AFTER the rounding)
    against the rule.  The rows before the rounding are not read back: every wv0 in (wv - rpg, wv] that the rule rounds to
    wv is tried, and one of them must give the read-back exactly.  Returns the list of candidates for the message."""
    tried = []
    for wv0 in range(max(1, wv - 15), wv + 1):
        p = plan(wu, wv0, big, Dv)
        if p["wv"] != wv:
            continue
        tried.append(p)
        if all(p[k] == got[k] for k in ("wp", "per", "rpg", "groups", "chunks")):
            return True, tried
    return False, tried


def emitted_pitches(max_rows=2048):
    """every (wp, per, rpg) the rule can emit for wu in 1..64, with the (wu, wv) that first gives it"""
    out = {}
    for wu in range(1, MAX_UNITS + 1):
        for wv in range(1, max_rows + 1):
            wp = pitch(wu, wv)
            out.setdefault((wp,) + _lattice(wp), (wu, wv))
    return out
