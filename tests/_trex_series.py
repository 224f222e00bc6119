"""A time series on disk as the reference writes it, for the host adapters' drivers (tests/host/*_main)."""
import os

import numpy as np


def write_series(d, steps, shape=(16, 12, 10), tstart=3, cache=2, bricks=2):
    """a .trex series as MetaVolume::writeAll would lay it out with time steps: <files>.<TTTT>.<BB> per brick (bricks
    split along z), `steps` = list of [z][y][x] u8 volumes for tstart, tstart + 1, ..."""
    nx, ny, nz = shape
    bz = nz // bricks
    name = os.path.join(d, "series")
    lines = ["Data Set Name: series", "Data Set Files: %s" % name,
             "Number of Time Steps: %d, %d, %d" % (len(steps), tstart, tstart + len(steps) - 1),
             "Time Step Cache: %d" % cache, "Volume Size int: %d, %d, %d" % shape,
             "Volume Size float: 1, %f, %f" % (ny / nx, nz / nx), "Number of Sub Volumes: %d" % bricks]
    for b in range(bricks):
        lines += ["SubVolume {", "Size int: %d, %d, %d" % (nx, ny, bz), "Size float: 1, %f, %f" % (ny / nx, bz / nx),
                  "Pos int: 0, 0, %d" % (b * bz), "Pos float: 0, 0, %f" % (b * bz / nx), "}"]
    open(name + ".trex", "w").write("\n".join(lines) + "\n")
    for k, v in enumerate(steps):
        for b in range(bricks):
            np.ascontiguousarray(v[b * bz:(b + 1) * bz]).tofile("%s.%04d.%02d" % (name, tstart + k, b))
    return name + ".trex"
