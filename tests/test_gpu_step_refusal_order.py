"""The ORDER of the refusals of the stencil producers' entries (smk.h: the derive, the merge and the merge with H; their plain,
shard and block forms).  The neighbours pin every message; here each call carries TWO faults that are neighbours in its
entry's order of refusals, and the message must be that of the earlier one:

  smk_step_extremes_device, smk_block_extremes_device       kind -> d_words -> the kind's shard or block refusals -> (block)
                                                             the fields, or d_fields / nf != 1 / the scalar
  smk_derive_timestep_shard, smk_merge_timestep_shard       shard refusals -> d_words
  smk_upload_timestep_scalar_block_device                   block refusals -> the scalar -> d_words
  smk_upload_timestep_fields_block_device                   block refusals -> the fields -> d_words
  smk_upload_timestep_scalar_device                         stencil refusals -> NULL -> dtype -> sizes -> alignment
  smk_upload_timestep_fields_device, ..._fields_h_device    (H: flags ->) stencil refusals -> d_fields NULL -> count -> dtype ->
                                                             sizes -> per field
  smk_step_extremes_h_device                                flags -> d_words -> shard refusals
  smk_merge_timestep_h_shard                                flags -> shard refusals -> d_words
  smk_block_extremes_h_device                               d_words -> flags -> block refusals -> the fields
  smk_upload_timestep_fields_h_block_device                 flags -> block refusals -> the fields -> d_words

Left out: every pair with "more tiles than a grid holds" (the merges' shard and block entries raise it behind their fields or
their words): it takes a stored box of 2^31 tiles, some 2^40 voxels, which no device holds.  The binding rejects none of the
pairs below before the library sees them.

A 37x13x11 u8 volume; rank 0 of 2 with a halo of 3 and a ring of 3 slots for the shard and block entries, the unsharded context
of the same ring for the entries that take the whole volume.  nelts 4 for the merges (three fields, or two with H), nelts 3 for
the derive.  Every call is refused before any launch; the rings are unchanged behind them."""
import numpy as np
import pytest

import _step_merge_h_ref as H
import _tblend_ref as T
from _gpu_mem import dev_ptr as dev, words_buf
from _step_gpu import UndisturbedHalos, rank_context

pytestmark = pytest.mark.gpu
DIMS, NRANKS, HALO, RING = (37, 13, 11), 2, 3, 3
DERIVE, MERGE = 0, 1


def refused(calls, smk):
    for call, why in calls:
        with pytest.raises(smk.SmkError, match=why):
            call()


def test_the_earlier_refusal_speaks(gpu_renderer_factory, smk):
    from _scenes import push_scene
    F = H.fields("u8", 3, DIMS, 0)
    data4, grad = H.source_step(F[..., :2], 1)                      # two fields, G and H
    data3 = np.ascontiguousarray(data4[..., :3])
    held = [dev(np.ascontiguousarray(F[..., e])) for e in range(3)] + [dev(np.zeros(DIMS[::-1], np.float32))]
    ptrs = [h[0] for h in held[:3]]                                 # (byte fields: any address is aligned)
    flt = held[3][0]                                                # a float scalar: flt + 2 is not aligned
    w = words_buf()
    p = w.data_ptr()
    whole = smk.smk_block((0, 0, 0), DIMS)
    bad = (DIMS[0] + 1, DIMS[1], DIMS[2])
    cached = r"time step 99 \(the source\) is not cached"
    count_h = "1 fields for a series of nelts 4 with add_h 1: the fields are nelts - 1 - add_h = 2"

    def made(data, nranks):
        C = rank_context(gpu_renderer_factory, DIMS, data, grad, H.MODE[(data.shape[-1] - 2, 1)], 0, nranks, HALO, cap=RING, opts=(("kernel", 1),))
        push_scene(C, T.scene(np.ascontiguousarray(data[..., :3]), grad), upload=False)
        return C

    # ---- rank 0 of 2, nelts 4: the merge and the merge with H, from a step and from blocks
    C = made(data4, NRANKS)
    try:
        with UndisturbedHalos(C, downloads=False):
            refused((
                # smk_step_extremes_device, the merge's kind
                (lambda: C.step_extremes_device(7, 99, None), "smk_step_extremes_device: kind 7 is neither"),
                (lambda: C.step_extremes_device(MERGE, 99, None), "smk_step_extremes_device: d_words is NULL"),
                (lambda: C.step_extremes_device(MERGE, 99, p + 2), "smk_step_extremes_device: d_words is not aligned"),
                # smk_block_extremes_device, the merge's kind
                (lambda: C.block_extremes_device(7, ptrs, 0, None, None), "smk_block_extremes_device: kind 7 is neither"),
                (lambda: C.block_extremes_device(MERGE, ptrs, 0, None, None), "smk_block_extremes_device: d_words is NULL"),
                (lambda: C.block_extremes_device(MERGE, None, 0, None, p), "smk_block_extremes_device: block is NULL"),
                (lambda: C.block_extremes_device(MERGE, None, 1, whole, p), "smk_block_extremes_device: d_fields is NULL"),
                (lambda: C.block_extremes_device(MERGE, ptrs[:1], 1, whole, p), "1 fields for a series of nelts 4: the fields are nelts - 1 = 3"),
                (lambda: C.block_extremes_device(MERGE, [ptrs[0], None, ptrs[2]], 1, whole, p), r"field_dtype 1 is not the ring's type \(0\)"),
                # smk_merge_timestep_shard
                (lambda: C.merge_timestep_shard(99, 5, None), "smk_merge_timestep_shard: " + cached),
                # smk_upload_timestep_fields_block_device
                (lambda: C.upload_timestep_fields_block_device(1, None, 0, None, p), "smk_upload_timestep_fields_block_device: block is NULL"),
                (lambda: C.upload_timestep_fields_block_device(1, ptrs[:1], 0, whole, None), "1 fields for a series of nelts 4: the fields are nelts - 1 = 3"),
                (lambda: C.upload_timestep_fields_block_device(1, [ptrs[0], None, ptrs[2]], 0, whole, None), r"d_fields\[1\] is NULL"),
                # smk_step_extremes_h_device
                (lambda: C.step_extremes_h_device(99, None, add_h=2), "smk_step_extremes_h_device: add_h 2 is neither 0 nor 1"),
                (lambda: C.step_extremes_h_device(99, None), "smk_step_extremes_h_device: d_words is NULL"),
                (lambda: C.step_extremes_h_device(99, p + 2), "smk_step_extremes_h_device: d_words is not aligned"),
                # smk_merge_timestep_h_shard
                (lambda: C.merge_timestep_h_shard(99, 5, None, blur=2), "smk_merge_timestep_h_shard: blur 2 is neither 0 nor 1"),
                (lambda: C.merge_timestep_h_shard(99, 5, None), "smk_merge_timestep_h_shard: " + cached),
                # smk_block_extremes_h_device
                (lambda: C.block_extremes_h_device(ptrs[:1], 0, whole, None, add_h=3), "smk_block_extremes_h_device: d_words is NULL"),
                (lambda: C.block_extremes_h_device(ptrs[:1], 0, None, p, add_h=3), "smk_block_extremes_h_device: add_h 3 is neither 0 nor 1"),
                (lambda: C.block_extremes_h_device(None, 0, None, p), "smk_block_extremes_h_device: block is NULL"),
                (lambda: C.block_extremes_h_device(None, 1, whole, p), "smk_block_extremes_h_device: d_fields is NULL"),
                (lambda: C.block_extremes_h_device(ptrs[:1], 1, whole, p), count_h),
                (lambda: C.block_extremes_h_device([ptrs[0], None], 1, whole, p), r"field_dtype 1 is not the ring's type \(0\)"),
                # smk_upload_timestep_fields_h_block_device
                (lambda: C.upload_timestep_fields_h_block_device(1, ptrs[:2], 0, None, p, blur=-1), "fields_h_block_device: blur -1 is neither 0 nor 1"),
                (lambda: C.upload_timestep_fields_h_block_device(1, None, 0, None, p), "smk_upload_timestep_fields_h_block_device: block is NULL"),
                (lambda: C.upload_timestep_fields_h_block_device(1, ptrs[:1], 0, whole, None), count_h),
                (lambda: C.upload_timestep_fields_h_block_device(1, [ptrs[0], None], 0, whole, None), r"d_fields\[1\] is NULL"),
                # the entries of the whole volume: a sharded context before anything of the data
                (lambda: C.upload_timestep_fields_device(1, None, 0, bad), "smk_upload_timestep_fields_device: a sharded context"),
                (lambda: C.upload_timestep_fields_h_device(1, None, 0, bad, add_h=2), "smk_upload_timestep_fields_h_device: add_h 2 is neither 0 nor 1"),
                (lambda: C.upload_timestep_fields_h_device(1, None, 0, bad), "smk_upload_timestep_fields_h_device: a sharded context")), smk)
        assert (w.cpu().numpy() == 0x5a5a5a5a).all(), "a refused export writes no word"
    finally:
        C.close()

    # ---- rank 0 of 2, nelts 3: the derive, from a step and from a block
    C = made(data3, NRANKS)
    try:
        with UndisturbedHalos(C, downloads=False):
            refused((
                (lambda: C.step_extremes_device(DERIVE, 99, None), "smk_step_extremes_device: d_words is NULL"),
                (lambda: C.block_extremes_device(DERIVE, ptrs[:1], 0, None, None), "smk_block_extremes_device: d_words is NULL"),
                (lambda: C.block_extremes_device(DERIVE, None, 0, None, p), "smk_block_extremes_device: block is NULL"),
                (lambda: C.block_extremes_device(DERIVE, None, 7, whole, p), "smk_block_extremes_device: d_fields is NULL"),
                (lambda: C.block_extremes_device(DERIVE, [None, ptrs[1]], 7, whole, p), "2 fields: the derive takes one scalar"),
                (lambda: C.block_extremes_device(DERIVE, [None], 7, whole, p), "smk_block_extremes_device: d_scalar is NULL"),
                (lambda: C.block_extremes_device(DERIVE, [flt + 2], 7, whole, p), "scalar_dtype 7 is none of"),
                (lambda: C.derive_timestep_shard(99, 5, None), "smk_derive_timestep_shard: " + cached),
                (lambda: C.upload_timestep_scalar_block_device(1, None, 0, None, p), "smk_upload_timestep_scalar_block_device: block is NULL"),
                (lambda: C.upload_timestep_scalar_block_device(1, None, 7, whole, None), "smk_upload_timestep_scalar_block_device: d_scalar is NULL"),
                (lambda: C.upload_timestep_scalar_block_device(1, flt + 2, 7, whole, None), "scalar_dtype 7 is none of"),
                (lambda: C.upload_timestep_scalar_block_device(1, flt + 2, 1, whole, None), "d_scalar is not aligned to its 4-byte elements"),
                (lambda: C.upload_timestep_scalar_device(1, None, 0, bad), "smk_upload_timestep_scalar_device: a sharded context")), smk)
        assert (w.cpu().numpy() == 0x5a5a5a5a).all(), "a refused export writes no word"
    finally:
        C.close()

    # ---- the unsharded context, nelts 4: the merges of dense fields of the whole volume
    C = made(data4, 1)
    try:
        with UndisturbedHalos(C, downloads=False):
            refused((
                (lambda: C.upload_timestep_fields_device(1, None, 1, bad), "smk_upload_timestep_fields_device: d_fields is NULL"),
                (lambda: C.upload_timestep_fields_device(1, ptrs[:2], 1, bad), "2 fields for a series of nelts 4: the fields are nelts - 1 = 3"),
                (lambda: C.upload_timestep_fields_device(1, ptrs, 1, bad), r"field_dtype 1 is not the ring's type \(0\)"),
                (lambda: C.upload_timestep_fields_device(1, [ptrs[0], None, ptrs[2]], 0, bad), "sizes 38x13x11 differ from the series' 37x13x11"),
                (lambda: C.upload_timestep_fields_h_device(1, None, 1, bad, blur=2), "smk_upload_timestep_fields_h_device: blur 2 is neither 0 nor 1"),
                (lambda: C.upload_timestep_fields_h_device(1, None, 1, bad), "smk_upload_timestep_fields_h_device: d_fields is NULL"),
                (lambda: C.upload_timestep_fields_h_device(1, ptrs[:1], 1, bad), count_h),
                (lambda: C.upload_timestep_fields_h_device(1, ptrs[:2], 1, bad), r"field_dtype 1 is not the ring's type \(0\)"),
                (lambda: C.upload_timestep_fields_h_device(1, [ptrs[0], None], 0, bad), "sizes 38x13x11 differ from the series' 37x13x11")), smk)
    finally:
        C.close()

    # ---- the unsharded context, nelts 3: the derive of a dense scalar of the whole volume
    C = made(data3, 1)
    try:
        with UndisturbedHalos(C, downloads=False):
            refused((
                (lambda: C.upload_timestep_scalar_device(1, None, 7, bad), "smk_upload_timestep_scalar_device: d_scalar is NULL"),
                (lambda: C.upload_timestep_scalar_device(1, flt + 2, 7, bad), "scalar_dtype 7 is none of"),
                (lambda: C.upload_timestep_scalar_device(1, flt + 2, 1, bad), "sizes 38x13x11 differ from the series' 37x13x11"),
                (lambda: C.upload_timestep_scalar_device(1, flt + 2, 1, DIMS), "d_scalar is not aligned to its 4-byte elements")), smk)
    finally:
        C.close()
    del held
