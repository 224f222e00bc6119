"""Sort-last compositing across ranks.

The reference has no distributed code: its only decomposition is MetaVolume::brick's spatial
grid drawn serially in visibility order on one GPU (MetaVolume.cpp:1369-1452,
NV20VolRen3D.cpp:190-231).  Here each rank owns a convex union of bricks (smk_set_shard),
ray-marches the full viewport against it, and the partial premultiplied-RGBA images are merged
with ONE exchange step:

    direct-send all-to-all of 1/P image tiles  ->  ordered "over" of P layers  ->  gather

First-hit depth (optional) travels beside the RGBA: a [npix_padded] float plane per rank, its
pieces sent with the RGBA pieces, merged by minimum (every blend mode: each rank reports its
nearest contributing sample, so the nearest over the ranks is the unsharded frame's depth).

"over" is associative but not commutative, so this cannot be an all-reduce(sum); the layer
order is the BSP front-to-back order of the shards for the current eye point.  On MI355X
`backend="nccl"` is RCCL over xGMI; the all-to-all uses all 7 links of each GPU at once.
The compositor is a parameter: the product passes the HIP kernel (smk_composite_over_device);
the gloo tests on CPU pass their own checker, so the same plumbing is exercised without a GPU.
"""
import torch
import torch.distributed as dist


def shard_region(dims, rank, nranks):
    """Mirror of the C++ rule in smk_set_shard: bit 0 of the rank splits x, bit 1 y, bit 2 z at
    the midpoint (the MetaVolume::brick 2x2x2 grid).  Returns (g0, g1) voxel index bounds."""
    g0, g1 = [0, 0, 0], list(dims)
    bit, n = 0, nranks
    while n > 1:
        a, half = bit % 3, dims[bit % 3] // 2
        if (rank >> bit) & 1:
            g0[a] = max(g0[a], half)
        else:
            g1[a] = min(g1[a], half)
        n >>= 1
        bit += 1
    return tuple(g0), tuple(g1)


def front_to_back_order(eye_voxel, dims, nranks):
    """BSP visibility order of the shards for an eye at `eye_voxel` (voxel index space): per
    split axis the half containing the eye comes first.  Agrees with the reference's
    centre-distance sort for equal bricks (NV20VolRen3D.cpp:195-212) and is exact for every ray."""
    near = [1 if eye_voxel[a] >= dims[a] // 2 - 0.5 else 0 for a in range(3)]
    nbits = nranks.bit_length() - 1
    keyed = []
    for r in range(nranks):
        key = 0
        for bit in range(nbits):
            if ((r >> bit) & 1) != near[bit % 3]:
                key |= 1 << bit
        keyed.append((key, r))
    return [r for _, r in sorted(keyed)]


def tile_pixels(npix, nranks):
    """pixels per rank tile (the frame is padded up to a multiple of nranks)"""
    return (npix + nranks - 1) // nranks


def _all_to_all(partial, recv, group, via_host):
    if via_host and partial.is_cuda:
        send = partial.cpu()
        got = torch.empty_like(send)
        dist.all_to_all_single(got, send, group=group)
        return got.to(partial.device)
    if recv is None:
        recv = torch.empty_like(partial)
    dist.all_to_all_single(recv, partial, group=group)
    return recv


def merge_depth(dlayers):
    """[P, tile] first-hit depths -> [tile]: the minimum over the layers (+inf where none is finite)"""
    out = dlayers[0]
    for l in range(1, dlayers.shape[0]):
        out = torch.minimum(out, dlayers[l])
    return out


def exchange_and_composite(partial, order, compositor, group=None, recv=None, via_host=False, depth=None, recv_depth=None):
    """partial: [npix_padded, 4] premultiplied RGBA of THIS rank's shard (npix_padded divisible
    by the world size).  Returns this rank's finished tile [npix_padded/P, 4].  `recv` lets a
    caller keep one receive buffer per frame slot; `via_host` stages device tensors through host
    memory for a backend that only moves CPU tensors (gloo rehearsals of the GPU plumbing).
    depth: [npix_padded] float first-hit depth of this rank's shard (+inf: no sample), or None.
    With it, its pieces travel with the RGBA pieces (`recv_depth`: the caller's receive buffer)
    and the result is (tile, tile_depth), tile_depth = the minimum over the ranks' pieces."""
    P = dist.get_world_size(group)
    n = partial.shape[0]
    assert n % P == 0
    # direct send: piece r of my partial image goes to rank r; I receive piece `me` of everyone
    recv = _all_to_all(partial, recv, group, via_host)
    layers = recv.view(P, n // P, 4)
    if depth is None:
        return compositor(layers, order)
    assert depth.shape[0] == n
    recv_depth = _all_to_all(depth, recv_depth, group, via_host)
    return compositor(layers, order), merge_depth(recv_depth.view(P, n // P))


def gather_frame(tile, dst=0, group=None, via_host=False, into=None, depth=None, depth_into=None):
    """finished tiles -> full frame on rank dst ([npix_padded,4]); None elsewhere.  `into` (rank dst):
    a preallocated [P, tile, 4] buffer the tiles are received into (no allocation per frame).
    depth: this rank's finished depth tile [tile] (exchange_and_composite's second result), or
    None; with it the result is (frame, frame_depth [npix_padded]) on rank dst, (None, None)
    elsewhere (`depth_into`: a preallocated [P, tile] buffer, as `into`)."""
    if depth is not None:
        d = _gather(depth, dst, group, via_host, depth_into)
        return _gather(tile, dst, group, via_host, into, 4), d
    return _gather(tile, dst, group, via_host, into, 4)


def _gather(tile, dst, group, via_host, into, comps=None):
    P = dist.get_world_size(group)
    me = dist.get_rank(group)
    src = tile.cpu() if via_host and tile.is_cuda else tile
    out = None
    if me == dst:
        if into is not None and not (via_host and tile.is_cuda):
            out = list(into.unbind(0))
        else:
            out = [torch.empty_like(src) for _ in range(P)]
    dist.gather(src, out, dst=dst, group=group)
    if me != dst:
        return None
    shape = (-1, comps) if comps else (-1,)
    if into is not None and not (via_host and tile.is_cuda):
        return into.view(*shape)
    return torch.cat(out, 0).to(tile.device)


class Pipeline:
    """Frames back to back with two in flight: while frame i's layers cross xGMI and are merged,
    frame i+1 is already ray-marching.  Each slot has its own stream and buffers; the renderer
    context itself is used by one frame at a time (frame i+1's launch waits for frame i's
    ray-marcher, not for its exchange).  `render(ptr, stream_handle)` ray-marches this rank's
    shard into the [npix_padded,4] buffer at `ptr`; `compositor(layers, order, out, stream_handle)`
    merges [P, tile, 4] front to back into `out`.
    depth=True: every frame also carries first-hit depth -- render(ptr, stream_handle, depth_ptr)
    writes the [npix_padded] depth plane beside the layer, frame(out, order, out_depth) delivers the
    merged depth (the minimum over the ranks) into out_depth ([npix]) on rank 0, and frame_check is
    called with the depth pointer as a fourth argument."""

    def __init__(self, render, compositor, npix, group=None, slots=2, via_host=False, frame_check=None, depth=False):
        """frame_check(token, ptr, stream_handle) -> bool (token = what render() returned), called once a frame's ray-marcher has finished and
        BEFORE its layer is exchanged: True = the frame was invalid and has been rendered again into
        the same buffer (the product passes Renderer.frame_failed + a gather-kernel re-render).  The
        repair is local to the rank, so no rank ever leaves the others waiting in a collective."""
        self.render, self.compositor, self.group, self.via_host = render, compositor, group, via_host
        self.frame_check = frame_check
        self.depth = depth
        P = dist.get_world_size(group)
        me = dist.get_rank(group)
        tp = tile_pixels(npix, P)
        self.npix = npix
        self.slots = []
        for _ in range(slots):
            self.slots.append({
                "stream": torch.cuda.Stream(),
                "partial": torch.zeros((tp * P, 4), dtype=torch.float32, device="cuda"),
                "recv": torch.empty((tp * P, 4), dtype=torch.float32, device="cuda"),
                "tile": torch.zeros((tp, 4), dtype=torch.float32, device="cuda"),
                # rank 0: where the finished tiles of a frame are gathered (allocated once)
                "full": torch.empty((P, tp, 4), dtype=torch.float32, device="cuda") if me == 0 else None})
            if depth:
                self.slots[-1].update({
                    "dpartial": torch.full((tp * P,), float("inf"), dtype=torch.float32, device="cuda"),
                    "drecv": torch.empty((tp * P,), dtype=torch.float32, device="cuda"),
                    "dfull": torch.empty((P, tp), dtype=torch.float32, device="cuda") if me == 0 else None})
        self.count = 0
        self.repaired = 0        # frames frame_check had to render again
        self.marched = None      # event: the latest frame's ray-marcher has finished
        self.delivered = None    # event: the latest frame has been copied into the caller's buffer
        self.pending = None      # the frame whose layer has not been exchanged yet

    def frame(self, out, order, out_depth=None):
        """enqueue one frame; on rank 0 `out` ([npix,4]) receives it (and `out_depth` ([npix]) its
        depth, depth=True).  Returns at once.  The frame's
        layer is exchanged when the NEXT frame has been enqueued (or at drain()): its ray-marcher has
        then had a frame's time to run, so looking at its status costs the host no wait to speak of,
        and the exchange still overlaps the next frame's ray-marching."""
        sl = self.slots[self.count % len(self.slots)]
        self.count += 1
        s = sl["stream"]
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            if self.marched is not None:
                s.wait_event(self.marched)
            dargs = (sl["dpartial"].data_ptr(),) if self.depth else ()
            sl["token"] = self.render(sl["partial"].data_ptr(), s.cuda_stream, *dargs)   # (whatever identifies the frame to frame_check)
            self.marched = torch.cuda.Event()
            self.marched.record(s)
        sl["marched"], sl["out"], sl["order"], sl["out_depth"] = self.marched, out, order, out_depth
        prev, self.pending = self.pending, sl
        if prev is not None:
            self._exchange(prev)

    def _exchange(self, sl):
        s = sl["stream"]
        with torch.cuda.stream(s):
            if self.frame_check is not None:
                sl["marched"].synchronize()
                dargs = (sl["dpartial"].data_ptr(),) if self.depth else ()
                if self.frame_check(sl["token"], sl["partial"].data_ptr(), s.cuda_stream, *dargs):
                    self.repaired += 1

            def comp(layers, order_):
                self.compositor(layers, order_, sl["tile"], s.cuda_stream)
                return sl["tile"]
            if self.depth:
                tile, dtile = exchange_and_composite(sl["partial"], sl["order"], comp, self.group, sl["recv"], self.via_host,
                                                     depth=sl["dpartial"], recv_depth=sl["drecv"])
                full, dfull = gather_frame(tile, 0, self.group, self.via_host, into=sl["full"], depth=dtile, depth_into=sl["dfull"])
            else:
                tile = exchange_and_composite(sl["partial"], sl["order"], comp, self.group, sl["recv"], self.via_host)
                full, dfull = gather_frame(tile, 0, self.group, self.via_host, into=sl["full"]), None
            if full is not None:
                if self.delivered is not None:
                    s.wait_event(self.delivered)
                sl["out"].copy_(full[:self.npix])
                if dfull is not None and sl["out_depth"] is not None:
                    sl["out_depth"].copy_(dfull[:self.npix])
                self.delivered = torch.cuda.Event()
                self.delivered.record(s)

    def drain(self):
        """exchange the last frame and make the caller's current stream wait for every frame enqueued so far"""
        if self.pending is not None:
            self._exchange(self.pending)
            self.pending = None
        for sl in self.slots:
            torch.cuda.current_stream().wait_stream(sl["stream"])


class ExchangePipeline:
    """Pipeline's contract with the merge behind the C ABI (smk_exchange_*, RCCL transport: grouped
    ncclSend/ncclRecv direct send, ordered over, gather -- csrc/smk_exchange.hip).  Python only
    sequences the calls; no torch collective is in the data path.  depth=True: as Pipeline's (the
    exchange carries depth from construction on: smk_exchange_partial_depth, smk_exchange_frame_depth)."""

    def __init__(self, render, exchange, npix, rank, frame_check=None, depth=False):
        self.render, self.x, self.npix, self.rank, self.frame_check = render, exchange, npix, rank, frame_check
        self.depth = depth
        if depth:
            self.x.partial_depth(0)
        self.count = 0
        self.repaired = 0
        self.pending = None

    def _dargs(self, slot):
        return (self.x.partial_depth(slot),) if self.depth else ()

    def frame(self, out, order=None, out_depth=None):
        slot = self.count & 1
        self.count += 1
        st = torch.cuda.current_stream().cuda_stream
        self.x.acquire(slot, st)
        token = self.render(self.x.partial(slot), st, *self._dargs(slot))
        self.x.rendered(slot, st)      # (also takes the shards' visibility order under THIS frame's camera)
        if order is not None:
            self.x.set_order(slot, order)
        ev = torch.cuda.Event()
        ev.record()
        prev, self.pending = self.pending, (slot, token, ev, out, out_depth)
        if prev is not None:
            self._exchange(prev)

    def _exchange(self, p):
        slot, token, ev, out, out_depth = p
        if self.frame_check is not None:
            ev.synchronize()
            st = torch.cuda.current_stream().cuda_stream
            if self.frame_check(token, self.x.partial(slot), st, *self._dargs(slot)):
                self.repaired += 1
                self.x.rendered(slot, st)
        if self.depth:
            self.x.frame_depth(slot, out.data_ptr() if self.rank == 0 else None, out_depth.data_ptr() if self.rank == 0 else None)
        else:
            self.x.frame(slot, out.data_ptr() if self.rank == 0 else None)

    def drain(self):
        if self.pending is not None:
            self._exchange(self.pending)
            self.pending = None
        self.x.wait(torch.cuda.current_stream().cuda_stream)


def render_shadow_frame_local(renderers, depth=False, scene_depth=None, scene_depth_kind=0):
    """One frame with shadows on P shard contexts of this process that share one device, ranks in order (smk.h "Shadows on
    shards"): phase 1 and the light exchange (smk_shadow_exchange_local), every rank's frame, then the HIP "over" of the P
    layers in smk_shard_order's order.  Returns the merged frame, a [H][W][4] float32 tensor on that device; depth=True:
    (frame, depth), depth the [H][W] minimum of the ranks' first-hit depths (smk_composite_over_depth_device).
    scene_depth: the host's opaque scene depth, [H][W] floats (array or tensor) of kind scene_depth_kind, the same
    full-window buffer for every rank (smk_render_occluded_device); the light exchange is not affected."""
    from .binding import shadow_exchange_local
    nranks = len(renderers)
    w, h = renderers[0].size
    npix = w * h
    dev = torch.device("cuda", renderers[0].device)
    shadow_exchange_local(renderers)
    layers = torch.zeros((nranks, npix, 4), dtype=torch.float32, device=dev)
    out = torch.zeros((npix, 4), dtype=torch.float32, device=dev)
    dlayers = torch.full((nranks, npix), float("inf"), dtype=torch.float32, device=dev) if depth else None
    dout = torch.empty((npix,), dtype=torch.float32, device=dev) if depth else None
    zs = None
    if scene_depth is not None:
        zs = torch.as_tensor(scene_depth, dtype=torch.float32).to(dev).contiguous()
        if tuple(zs.shape) != (h, w):
            raise ValueError("scene_depth must be [%d][%d] floats, got shape %s" % (h, w, tuple(zs.shape)))
    torch.cuda.synchronize(dev)
    for r, R in enumerate(renderers):
        R.render_device(layers[r].data_ptr(), dlayers[r].data_ptr() if depth else None,
                        d_scene_depth=zs.data_ptr() if zs is not None else None, scene_depth_kind=scene_depth_kind)
    torch.cuda.synchronize(dev)
    order = renderers[0].shard_order(nranks)
    if depth:
        renderers[0].composite_over_depth_device(layers.data_ptr(), dlayers.data_ptr(), nranks, order, npix, out.data_ptr(), dout.data_ptr())
    else:
        renderers[0].composite_over_device(layers.data_ptr(), nranks, order, npix, out.data_ptr())
    torch.cuda.synchronize(dev)
    return (out.view(h, w, 4), dout.view(h, w)) if depth else out.view(h, w, 4)


def stencil_timestep_local(renderers, kind, src, out, compat=1, blur=0, stream=None, words=None, add_h=1):
    """Step `out` becomes the derived (kind "derive"), merged (kind "merge") or merged-with-H (kind "merge_h") step of the cached
    step `src` on P shard contexts of this process that share one device, ranks in order (smk.h, "The two stencil producers on a
    SHARDED context"): every rank exports the extremes of its region (smk_step_extremes_device; "merge_h":
    smk_step_extremes_h_device), the eight words combine by elementwise integer maximum, and every rank runs the write pass
    with the combined words (smk_derive_timestep_shard / smk_merge_timestep_shard / smk_merge_timestep_h_shard).  No voxel
    moves between ranks.  A multi-process host does the same with one integer MAX all-reduce of 8 words in place of the
    maximum taken here.
    The stencil reaches 2 voxels for "derive" and for "merge_h" (whatever add_h and blur are), 1 voxel for "merge": the source
    needs a valid halo of the reach + 1, and the result's is the source's less the reach.
    add_h: "merge_h" alone -- 1: the channel behind G is H of the summed gradient; 0: no H (blur then gives smoothed normals
    to a merge without H).  compat and blur: "derive" and "merge_h"; "merge" has neither.
    stream: a hipStream_t handle for every rank's kernels (an int or a ctypes.c_void_p).  Exports, the maximum and the write
    passes are then all enqueued on it and the host waits for nothing.  None: each context's own stream; the host then waits
    once for the ranks' exports and once for the combined words, both waits the combine's; the write passes are enqueued and
    not waited for.
    words: a [P + 1][8] int32 tensor on the device to work in (rows 0..P-1 the ranks' exports, row P the combined words), or
    None to have one made.  It is returned, and must stay alive until the streams have passed the write passes."""
    from .binding import EXTREMES_DERIVE, EXTREMES_MERGE
    if kind not in ("derive", "merge", "merge_h"):
        raise ValueError("kind must be 'derive', 'merge' or 'merge_h', got %r" % (kind,))
    nranks = len(renderers)
    dev = torch.device("cuda", renderers[0].device)
    if words is None:
        words = torch.empty((nranks + 1, 8), dtype=torch.int32, device=dev)
    if tuple(words.shape) != (nranks + 1, 8) or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError("words must be a contiguous [%d][8] int32 tensor" % (nranks + 1))
    k = EXTREMES_DERIVE if kind == "derive" else EXTREMES_MERGE
    for r, R in enumerate(renderers):
        if kind == "merge_h":
            R.step_extremes_h_device(src, words[r].data_ptr(), add_h=add_h, compat=compat, stream=stream)
        else:
            R.step_extremes_device(k, src, words[r].data_ptr(), compat=compat, stream=stream)
    if stream is None:
        torch.cuda.synchronize(dev)  # the combine's wait: every rank's export, each on its context's stream, is in memory
        words[nranks].copy_(words[:nranks].amax(0))
        torch.cuda.current_stream(dev).synchronize()  # ... and the combined words, before the contexts' streams read them
    else:
        handle = stream.value if hasattr(stream, "value") else int(stream)
        with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=dev)):  # behind the exports, before the write passes
            words[nranks].copy_(words[:nranks].amax(0))
    for R in renderers:
        if kind == "derive":
            R.derive_timestep_shard(src, out, words[nranks].data_ptr(), compat=compat, blur=blur, stream=stream)
        elif kind == "merge_h":
            R.merge_timestep_h_shard(src, out, words[nranks].data_ptr(), add_h=add_h, compat=compat, blur=blur, stream=stream)
        else:
            R.merge_timestep_shard(src, out, words[nranks].data_ptr(), stream=stream)
    return words


def stencil_block_local(renderers, kind, blocks, out, compat=1, blur=0, stream=None, words=None, add_h=1):
    """stencil_timestep_local from the ranks' OWN dense blocks of the volume in place of a cached step (smk.h, "Blocks of a
    decomposed simulation"): step `out` becomes the derived (kind "derive"), merged (kind "merge") or merged-with-H (kind
    "merge_h") step of the scalar or the fields every rank holds for its sub-domain, ghost cells included.  blocks: per rank
    (ptrs, dtype, block) -- the device addresses of the dense arrays (one scalar for the derive, nelts - 1 fields for the merge,
    nelts - 1 - add_h for the merge with H), their dtype code and the smk_block() that lays all of them out.  Every rank
    exports the extremes of its region (smk_block_extremes_device; "merge_h": smk_block_extremes_h_device), the eight words
    combine by elementwise integer maximum, and every rank runs the write pass with the combined words
    (smk_upload_timestep_scalar_block_device / smk_upload_timestep_fields_block_device /
    smk_upload_timestep_fields_h_block_device).  No voxel moves between ranks, and no rank sees an array it does not hold.  A
    multi-process host does the same with one integer MAX all-reduce of 8 words.
    The reach is stencil_timestep_local's: 2 voxels for "derive" and "merge_h", 1 for "merge"; the blocks' ghost cells must give
    a valid halo of the reach + 1.  add_h: as there.
    stream, words and the return value: as stencil_timestep_local; `stream` also orders the reads of the blocks."""
    from .binding import EXTREMES_DERIVE, EXTREMES_MERGE
    if kind not in ("derive", "merge", "merge_h"):
        raise ValueError("kind must be 'derive', 'merge' or 'merge_h', got %r" % (kind,))
    nranks = len(renderers)
    if len(blocks) != nranks:
        raise ValueError("%d blocks for %d ranks" % (len(blocks), nranks))
    dev = torch.device("cuda", renderers[0].device)
    if words is None:
        words = torch.empty((nranks + 1, 8), dtype=torch.int32, device=dev)
    if tuple(words.shape) != (nranks + 1, 8) or words.dtype != torch.int32 or not words.is_contiguous():
        raise ValueError("words must be a contiguous [%d][8] int32 tensor" % (nranks + 1))
    k = EXTREMES_DERIVE if kind == "derive" else EXTREMES_MERGE
    for r, (R, (ptrs, dtype, block)) in enumerate(zip(renderers, blocks)):
        if kind == "merge_h":
            R.block_extremes_h_device(ptrs, dtype, block, words[r].data_ptr(), add_h=add_h, compat=compat, stream=stream)
        else:
            R.block_extremes_device(k, ptrs, dtype, block, words[r].data_ptr(), compat=compat, stream=stream)
    if stream is None:
        torch.cuda.synchronize(dev)  # the combine's wait: every rank's export, each on its context's stream, is in memory
        words[nranks].copy_(words[:nranks].amax(0))
        torch.cuda.current_stream(dev).synchronize()  # ... and the combined words, before the contexts' streams read them
    else:
        handle = stream.value if hasattr(stream, "value") else int(stream)
        with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=dev)):  # behind the exports, before the write passes
            words[nranks].copy_(words[:nranks].amax(0))
    for R, (ptrs, dtype, block) in zip(renderers, blocks):
        if kind == "derive":
            R.upload_timestep_scalar_block_device(out, ptrs[0], dtype, block, words[nranks].data_ptr(), compat=compat, blur=blur, stream=stream)
        elif kind == "merge_h":
            R.upload_timestep_fields_h_block_device(out, ptrs, dtype, block, words[nranks].data_ptr(), add_h=add_h, compat=compat, blur=blur,
                                                    stream=stream)
        else:
            R.upload_timestep_fields_block_device(out, ptrs, dtype, block, words[nranks].data_ptr(), stream=stream)
    return words


def refill_halo_local(renderers, step, stream=None):
    """The stored halo of cached step `step` (an id, or binding.STEP_CURRENT) on P shard contexts of this process, ranks in
    order, copied bit for bit from the ranks that own those voxels (smk.h, "Halo refill"; smk_step_halo_exchange_local).  After
    stencil_timestep_local or stencil_block_local a step's valid halo is the source's less the reach and the stored voxels
    beyond it are a rim of zeros; after this call the step is the unsharded step's voxels on the whole stored box, with valid
    halo = option "halo": frames with shadows or perturbation, the probe and later producers treat it as an uploaded step.
    stream: a hipStream_t handle (an int or a ctypes.c_void_p) on which everything is enqueued, the host waiting for
    nothing; None: every context's own stream, and the host waits for all of them.  A multi-process host does the same with
    Renderer.step_halo_layout, step_halo_exports_device, one all-to-all-v of the segments, and step_halo_entries_device."""
    from .binding import step_halo_exchange_local
    step_halo_exchange_local(renderers, step, stream)
