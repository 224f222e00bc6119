"""The slice-ring kernel's instance table (smk_slab.h slab_inst_missing / slab_inst_part) against the library that was built
from it: tests/host/slab_inst_main prints the table for the full cross product of keys, and the host side of libsmk_hip.so
keeps every kernel's mangled name for registration -- the two sets must be the same, nothing missing and nothing extra."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "slab_inst_main")
LIB = os.path.join(ROOT, "simian-spacemonkey_amd", "csrc", "libsmk_hip.so")
NAME = re.compile(rb"_Z10smk_k_slabI((?:L[ib]\d+E)+)Ev12RenderParams10SlabParams")
# instances per translation unit (SLAB_PART 0..7), recorded from the build of the commit before the table existed: u8, f32
# (+ 9 diagnostic), shadows, scene depth, scene depth + shadows, NV20 look, u16, u16 shadows
PER_PART = [117, 126, 144, 126, 72, 132, 114, 72]

U16_LEFT_OUT = "u16 voxels have no 10+2-wave instances with NV20 shading, the 3-D table and brick flags (they would spill)"
NV20_LEFT_OUT = "option shadow_look 1 has no float-voxel 10+2-wave instances with brick flags (they would spill)"
U16_NO_OCC = "u16 voxels have no scene-depth instances of the slice-ring kernel"
U16_NO_NV20 = "u16 voxels have no shadow_look 1 instances of the slice-ring kernel"
NV20_NO_OCC = "option shadow_look 1 has no scene-depth instances of the slice-ring kernel"
NO_COLOUR_TABLE = "no colour-table instance for this tile size"


@pytest.fixture(scope="module")
def table():
    """key (dt, sh, perm, nw, nl, diag, tf, br, shd, occ, nvl) -> ("built", part) or ("missing", reason)"""
    assert os.path.exists(EXE), "build with __graft_entry__.build()"
    out = subprocess.run([EXE], capture_output=True, text=True, check=True).stdout
    t = {}
    for line in out.splitlines():
        w = line.split(" ", 11)
        key = tuple(int(x) for x in w[:11])
        assert key not in t
        t[key] = ("built", int(w[11].split()[1])) if w[11].startswith("built ") else ("missing", w[11])
    return t


@pytest.fixture(scope="module")
def compiled():
    """the keys of the smk_k_slab instances in the library, decoded from their mangled names"""
    assert os.path.exists(LIB), "build with __graft_entry__.build()"
    names = set(m.group(0) for m in NAME.finditer(open(LIB, "rb").read()))
    keys = [tuple(int(a) for a in re.findall(rb"L[ib](\d+)E", NAME.match(n).group(1))) for n in names]
    assert all(len(k) == 11 for k in keys) and len(set(keys)) == len(names)
    return set(keys)


def test_the_table_covers_the_full_cross_product(table):
    assert len(table) == 3 * 3 * 3 * 3 * 3 * 32
    shapes = set(k[3:5] for k in table)
    assert shapes == {(8, 2), (10, 2), (12, 4)}
    for i, n in ((0, 3), (1, 3), (2, 3), (6, 3), (5, 2), (7, 2), (8, 2), (9, 2), (10, 2)):
        assert set(k[i] for k in table) == set(range(n))


def test_the_library_holds_exactly_the_instances_the_table_calls_built(table, compiled):
    built = set(k for k, v in table.items() if v[0] == "built")
    assert sorted(built - compiled) == [], "called built, not in the library"
    assert sorted(compiled - built) == [], "in the library, not called built"


def test_instances_per_part(table, compiled):
    parts = collections.Counter(table[k][1] for k in compiled if table.get(k, ("",))[0] == "built")
    assert [parts[p] for p in range(8)] == PER_PART
    assert len(compiled) == sum(PER_PART) == 903


#          dt sh perm nw nl diag tf br shd occ nvl
HOLES = [((2, 2, 0, 10, 2, 0, 2, 1, 0, 0, 0), U16_LEFT_OUT),     # u16, NV20 shading, 3-D table, 10+2 waves, brick flags
         ((2, 2, 2, 10, 2, 0, 2, 1, 0, 0, 0), U16_LEFT_OUT),
         ((1, 2, 1, 10, 2, 0, 1, 1, 1, 0, 1), NV20_LEFT_OUT),    # f32, NV20 look, 10+2 waves, brick flags
         ((1, 0, 0, 10, 2, 0, 2, 1, 1, 0, 1), NV20_LEFT_OUT),
         ((2, 0, 0, 8, 2, 0, 1, 1, 0, 1, 0), U16_NO_OCC),        # u16 with scene depth
         ((2, 1, 1, 12, 4, 0, 2, 1, 1, 1, 0), U16_NO_OCC),
         ((2, 2, 0, 8, 2, 0, 1, 0, 1, 0, 1), U16_NO_NV20),       # u16 in the NV20 look
         ((0, 2, 0, 8, 2, 0, 1, 1, 1, 1, 1), NV20_NO_OCC),       # the NV20 look with scene depth
         ((1, 0, 2, 12, 4, 0, 2, 1, 1, 1, 1), NV20_NO_OCC),
         ((0, 1, 0, 8, 2, 0, 0, 0, 0, 0, 0), NO_COLOUR_TABLE),   # the 1-D colour table, shaded
         ((1, 1, 2, 12, 4, 0, 0, 0, 0, 0, 0), NO_COLOUR_TABLE)]


@pytest.mark.parametrize("key,reason", HOLES)
def test_named_holes_and_their_reasons(table, compiled, key, reason):
    assert table[key] == ("missing", reason)
    assert key not in compiled


def test_the_neighbours_of_the_holes_are_built(table):
    """what the left-out rules must NOT take with them: the same instances without brick flags, and on the other shapes"""
    assert table[(2, 2, 0, 10, 2, 0, 2, 0, 0, 0, 0)] == ("built", 6)
    assert table[(2, 2, 0, 12, 4, 0, 2, 1, 0, 0, 0)] == ("built", 6)
    assert table[(0, 2, 0, 10, 2, 0, 2, 1, 0, 0, 0)] == ("built", 0)
    assert table[(1, 2, 1, 10, 2, 0, 1, 0, 1, 0, 1)] == ("built", 5)
    assert table[(0, 2, 1, 10, 2, 0, 1, 1, 1, 0, 1)] == ("built", 5)
    assert table[(1, 1, 0, 8, 2, 1, 1, 1, 0, 0, 0)] == ("built", 1)      # the diagnostic instance
