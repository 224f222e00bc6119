"""Inputs shared by the clip-slice tests (CPU checker tests, GPU tests, shards): the widget's corners for an orthogonal
plane, and poses for which the quad's coverage does not hinge on float32 against float64 edge decisions."""
import numpy as np

AXES = {1: "X+", 2: "X-", 3: "Y+", 4: "Y-", 5: "Z+", 6: "Z-"}
# the pass drawClip's switch gives (R8kVolRen3D.cpp:826-879 asked with dv before and -dv after the volume): per oaxis the
# pass for dv < 0 and for dv > 0 (1 before, 2 after)
PASS_TABLE = {1: (1, 2), 2: (2, 1), 3: (2, 1), 4: (1, 2), 5: (1, 2), 6: (2, 1)}
# trackball rotations (axis, degrees) under which every orthogonal plane is seen at an angle
POSES = {"rot": ((1, 1, 0), 30), "side": ((.2, 1, .1), 75), "diag": ((1, 1, 1), 50), "back": ((0, 1, 0), 160)}


def widget_corners(oaxis, vpos, fsize, margin=0.25):
    """gluvv.clip.corners of an orthogonal plane through vpos (CPWidgetRen::set_info, CPWidgetRen.cpp:281-294: the widget's
    rectangle, corner by corner round the ring, in volume space); margin > 0: wider than the volume, as the widget is
    (drawClip clamps it to the box), margin < 0: a rectangle inside the cut face"""
    a = (oaxis - 1) // 2
    b, c = [k for k in range(3) if k != a]
    fs = [float(f) for f in fsize]
    ring = [(-margin, -margin), (fs[b] + margin, -margin), (fs[b] + margin, fs[c] + margin), (-margin, fs[c] + margin)]
    out = np.zeros((4, 3), np.float32)
    for k, (u, v) in enumerate(ring):
        out[k, a], out[k, b], out[k, c] = vpos[a], u, v
    return out


def clip_vpos(oaxis, fsize, frac=0.45):
    """a plane position `frac` of the way along the clip axis (the other coordinates mid-volume)"""
    a = (oaxis - 1) // 2
    v = [float(f) * .5 for f in fsize]
    v[a] = float(fsize[a]) * frac
    return v

# The GPU tests' frames: SIZE x SIZE pixels, and per clip axis a pose under which no pixel centre of the plane's quad
# (margins 0.25 and -0.2, unit fSize) lies within 1e-3 px of a projected edge -- tests/test_clip_slice_ref.py checks it
SIZE = 64
CASE_POSE = {1: "rot", 2: "diag", 3: "diag", 4: "rot", 5: "side", 6: "rot"}
# every (oaxis, plane position as a fraction of fSize, margin) the GPU tests draw
GPU_QUADS = [(a, 0.45, 0.25) for a in sorted(AXES)] + [(5, 0.45, -0.2), (2, 1.3, 0.25)]
