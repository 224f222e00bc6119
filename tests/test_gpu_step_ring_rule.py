"""The ring's slot rule, one table for every producer of a resident time step (csrc/smk_internal.h, smk_step_produce;
smk.h smk_blend_timesteps, smk_derive_timestep, smk_merge_timestep, smk_upload_timestep_scalar_device,
smk_upload_timestep_fields_device).

The expectations come from the rule as it is stated, not from the code:
  - a call whose output id is cached overwrites that slot and never fails for lack of slots;
  - otherwise the output takes a slot that is neither a source's nor the current step's, so the call is refused exactly when
    the capacity is below 1 + the number of distinct slots among the sources and the current step, and the refusal names the
    entry, the capacity and that number;
  - after a successful call the ring lists the output, every source and the current step, at most `capacity` ids, and the
    current step is the one it was.
One geometry that all five producers accept: a 6x5x4 u8 volume of nelts 3 with normals.  What the producers write is the
business of test_gpu_tblend.py, test_gpu_step_derive.py and test_gpu_step_merge.py."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIMS = (6, 5, 4)                      # (sx, sy, sz)
A, B, THIRD, OUT = 0, 1, 2, 5         # the ids: the sources, a step that is neither source nor output, the output
WHO = {"blend": "smk_blend_timesteps", "derive": "smk_derive_timestep", "merge": "smk_merge_timestep",
       "scalar": "smk_upload_timestep_scalar_device", "fields": "smk_upload_timestep_fields_device"}


def sources(producer, same):
    return {"blend": [A, A] if same else [A, B], "derive": [A], "merge": [A]}.get(producer, [])


def cases():
    """(producer, capacity, where the current step stands, blend's a == b): every state that the capacity can hold"""
    out = []
    for producer in WHO:
        for same in ((False, True) if producer == "blend" else (False,)):
            src = sources(producer, same)
            for where in ("source", "output", "third"):
                if where == "source" and not src:
                    continue
                held = len(set(src)) + (where != "source")       # the sources, and the current step where it is none of them
                out += [(producer, cap, where, same) for cap in range(1, 5) if cap >= held]
    return out


def case_id(c):
    return "%s%s-cap%d-%s" % (c[0], "-aa" if c[3] else "", c[1], c[2])


@pytest.fixture(scope="module")
def steps():
    """per id the host arrays of a step, and the dense device arrays of the two upload entries (kept alive by the fixture)"""
    import torch
    nx, ny, nz = DIMS
    rng = np.random.default_rng(20)
    host = {i: (rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8), rng.integers(0, 256, (nz, ny, nx, 3), dtype=np.uint8))
            for i in (A, B, THIRD, OUT)}
    dense = [torch.from_numpy(rng.integers(0, 256, (nz, ny, nx), dtype=np.uint8)).cuda() for _ in range(2)]
    torch.cuda.synchronize()                                      # the dense arrays are on the device before a context reads them
    return host, dense


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_slot_rule(gpu_renderer_factory, smk, steps, case):
    producer, cap, where, same = case
    host, dense = steps
    src = sources(producer, same)
    cur = {"source": A, "output": OUT, "third": THIRD}[where]
    R = gpu_renderer_factory()
    try:
        R.set_timestep_cache(cap)
        for i in sorted(set(src + [cur])):                        # (the first upload is the current step until the selection)
            R.upload_timestep(i, *host[i])
        R.select_timestep(cur)
        before = R.timesteps()
        assert before == (cur, sorted(set(src + [cur])))

        def call():
            if producer == "blend":
                R.blend_timesteps(src[0], src[1], 0.3, OUT)
            elif producer == "derive":
                R.derive_timestep(A, OUT)
            elif producer == "merge":
                R.merge_timestep(A, OUT)
            elif producer == "scalar":
                R.upload_timestep_scalar_device(OUT, dense[0].data_ptr(), 0, DIMS)
            else:
                R.upload_timestep_fields_device(OUT, [d.data_ptr() for d in dense], 0, DIMS)

        need = 1 + len(set(src + [cur]))
        if where != "output" and cap < need:
            # (without a source the capacity is 1 and `need` 2: smk.h's text for that case spells the capacity out)
            what = (r"the cache holds %d steps\b.*\(here %d\)" % (cap, need) if src else
                    r"time step %d: the cache holds one step, the current one \(%d\)" % (OUT, cur))
            with pytest.raises(smk.SmkError, match="^" + re.escape(WHO[producer]) + ": " + what):
                call()
            assert R.timesteps() == before                        # a refused call changes nothing
        else:
            call()
            now, ids = R.timesteps()
            assert now == cur
            assert set(src + [cur, OUT]) <= set(ids) and len(ids) == len(set(ids)) <= cap, (ids, cap)
    finally:
        R.close()
