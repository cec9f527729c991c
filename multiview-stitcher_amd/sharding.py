"""One mosaic over the GPUs of a node: tile ownership, pair and chunk assignment.

Units are independent -- one task per image pair (registration.py:2657-2664) and one per output chunk
(fusion/_core.py:1133-1141; task shapes after browser/executors.py:166-194, 267-281) -- so the data path needs no
collective.  What has to be decided is WHERE each tile lives, so that it is uploaded once and its neighbours fetch it
once:

* the output stack is cut into one sub-box per rank (z first, then y, then x: z-major slabs keep a rank's chunks on the
  same tiles);
* a tile is OWNED by the rank whose sub-box holds its centre: with 8 ranks and the 4 x 4 x 4 grid every rank owns a
  2 x 2 x 2 brick of tiles;
* a pair inside a brick is registered by the brick's rank, a pair across two bricks by whichever of the two ranks has fewer
  pairs (`edge_owners`: 18 pairs per rank on the 4 x 4 x 4 grid over 8 ranks); an output chunk is fused by the rank whose
  sub-box it lies in;
* a rank therefore needs its own tiles plus a one-tile HALO: the partners of its pairs and every tile that reaches into
  its sub-box.  In one process (threads, one context per GPU) the halo arrives by peer copies (`DeviceArray.on_device` ->
  mvs_memcpy_peer, xGMI); with one process per GPU it is exchanged once by point-to-point sends (`exchange_halo`,
  torch.distributed isend / irecv = RCCL over xGMI).  Neither is on the per-step path: tiles stay resident.
* the pairwise results (a 4 x 4 matrix, a quality and a box per pair) are gathered on every rank
  (`ShardedPairExecutor`, all_gather_object: a few kB of control data) and the groupwise resolution runs replicated.
"""

from __future__ import annotations

import warnings

import numpy as np


def factor_ranks(world_size, extents):
    """Split counts (one per axis, product == world_size): factors of 2 (then odd factors) go to the axis whose parts are
    currently the longest, ties to the FIRST axis (z-major)."""
    counts = [1] * len(extents)
    n = int(world_size)
    factors = []
    p = 2
    while n > 1:
        while n % p == 0:
            factors.append(p)
            n //= p
        p += 1
    for f in sorted(factors, reverse=True):
        part = [e / c for e, c in zip(extents, counts)]
        k = int(np.argmax(part))      # argmax returns the first of equal maxima
        counts[k] *= f
    return counts


def output_subboxes(output_stack_properties, world_size, sdims=None):
    """Cut an output stack (dict-of-dicts origin / spacing / shape) into ``world_size`` voxel-aligned sub-boxes; returns the
    list of sub stacks (rank order: first axis slowest) and the split counts."""
    osp = output_stack_properties
    sdims = list(sdims or [d for d in ("z", "y", "x") if d in osp["shape"]])
    shape = [int(osp["shape"][d]) for d in sdims]
    counts = factor_ranks(world_size, shape)
    bounds = [np.linspace(0, n, c + 1).round().astype(int) for n, c in zip(shape, counts)]
    boxes = []
    for idx in np.ndindex(*counts):
        lo = [int(bounds[k][i]) for k, i in enumerate(idx)]
        hi = [int(bounds[k][i + 1]) for k, i in enumerate(idx)]
        boxes.append({
            "origin": {d: float(osp["origin"][d]) + lo[k] * float(osp["spacing"][d]) for k, d in enumerate(sdims)},
            "spacing": {d: float(osp["spacing"][d]) for d in sdims},
            "shape": {d: hi[k] - lo[k] for k, d in enumerate(sdims)},
            "index_offset": {d: lo[k] for k, d in enumerate(sdims)},
        })
    return boxes, counts


def _world_box(stack_props, affine, sdims):
    """Axis-aligned world bounding box of a view (corners of its stack under its affine)."""
    nd = len(sdims)
    o = np.array([float(stack_props["origin"][d]) for d in sdims])
    s = np.array([float(stack_props["spacing"][d]) for d in sdims])
    n = np.array([float(stack_props["shape"][d]) for d in sdims])
    corners = np.array(list(np.ndindex(*([2] * nd)))) * ((n - 1) * s) + o
    A = np.asarray(affine, dtype=np.float64)
    w = corners @ A[:nd, :nd].T + A[:nd, nd]
    return w.min(0), w.max(0)


def tile_owners(stack_props_list, affines, subboxes, sdims=None):
    """Owner rank of every view: the rank whose sub-box holds the centre of the view's world bounding box (clamped into the
    output stack)."""
    sdims = list(sdims or [d for d in ("z", "y", "x") if d in subboxes[0]["shape"]])
    los = np.array([[b["origin"][d] for d in sdims] for b in subboxes])
    his = np.array([[b["origin"][d] + b["shape"][d] * b["spacing"][d] for d in sdims] for b in subboxes])
    glo, ghi = los.min(0), his.max(0)
    owners = []
    for sp, a in zip(stack_props_list, affines):
        lo, hi = _world_box(sp, a, sdims)
        c = np.clip((lo + hi) / 2, glo, np.nextafter(ghi, glo))
        inside = np.all((c >= los) & (c < his), axis=1)
        owners.append(int(np.argmax(inside)))
    return owners


def edge_owners(edges, owners):
    """The rank that registers each pair.  A pair whose two views live on one rank stays there; a pair ACROSS two ranks goes, in edge
    order, to whichever of the two has fewer pairs so far (ties: the owner of the fixed view).  INVARIANT: the assignment is a function
    of the WHOLE ordered edge list, not of a pair alone -- ``rank_tiles`` (which puts the partners of a rank's assigned pairs into its
    halo) and ``ShardedPairExecutor`` must be given the same ordered list, the one ``register()`` produces after pruning; a halo
    derived from another pruning, a ``pairs=`` subset or a quality-filtered list does not hold the tiles this assignment needs (the
    executor then raises "voxels live on rank N").  Always handing it to the fixed view's owner (rounds 3-4) loaded the ranks 12 ... 24 pairs on the 4 x 4 x 4 grid
    over 8 ranks (the low corner brick owns the fixed view of every pair across its three inner faces); balanced it is 18 each, and
    the pairwise phase of a step lasts as long as its busiest rank.  Deterministic: every rank derives the same assignment."""
    load = {}
    for i, j in edges:
        if owners[i] == owners[j]:
            load[owners[i]] = load.get(owners[i], 0) + 1
    out = []
    for i, j in edges:
        a, b = owners[i], owners[j]
        if a == b:
            out.append(a)
            continue
        r = b if load.get(b, 0) < load.get(a, 0) else a
        load[r] = load.get(r, 0) + 1
        out.append(r)
    # the greedy pass fills early ranks first: move cross pairs from the fuller to the emptier of their two ranks until no move helps
    for _ in range(len(edges)):
        moved = False
        for k, (i, j) in enumerate(edges):
            a, b = owners[i], owners[j]
            if a == b:
                continue
            cur, other = out[k], (b if out[k] == a else a)
            if load[cur] > load.get(other, 0) + 1:
                load[cur] -= 1
                load[other] = load.get(other, 0) + 1
                out[k] = other
                moved = True
        if not moved:
            break
    return out


def rank_tiles(stack_props_list, affines, subboxes, edges, owners, rank, margin=8.0, sdims=None):
    """Views rank ``rank`` must hold: its own, the partners of the pairs it registers and every view whose world box (grown
    by ``margin`` world units: registration may move a view by a few pixels) reaches into its sub-box."""
    sdims = list(sdims or [d for d in ("z", "y", "x") if d in subboxes[0]["shape"]])
    need = {v for v, o in enumerate(owners) if o == rank}
    for (i, j), o in zip(edges, edge_owners(edges, owners)):
        if o == rank:
            need.update((i, j))
    b = subboxes[rank]
    blo = np.array([b["origin"][d] for d in sdims])
    bhi = np.array([b["origin"][d] + (b["shape"][d] - 1) * b["spacing"][d] for d in sdims])
    for v, (sp, a) in enumerate(zip(stack_props_list, affines)):
        lo, hi = _world_box(sp, a, sdims)
        if np.all(lo - margin <= bhi) and np.all(hi + margin >= blo):
            need.add(v)
    return sorted(need)


class RemoteArray:
    """Placeholder for the data of a view that lives on another rank: shape and dtype only.  Registration's graph
    building and the fuse planner read metadata; any attempt to touch the voxels raises."""

    def __init__(self, shape, dtype, owner=None):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.owner = owner

    ndim = property(lambda self: len(self.shape))
    size = property(lambda self: int(np.prod(self.shape)))

    def __getitem__(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        key = key + (slice(None),) * (self.ndim - len(key))
        shape = []
        for k, n in zip(key, self.shape):
            if isinstance(k, slice):
                lo, hi, _ = k.indices(n)
                shape.append(max(hi - lo, 0))
        return RemoteArray(shape, self.dtype, self.owner)

    def _fail(self, *a, **k):
        raise RuntimeError(f"this view's voxels live on rank {self.owner}: it is not part of this rank's tiles + halo")

    __array__ = get = astype = _fail
    ptr = property(_fail)


class ShardedPairExecutor:
    """``pairwise_executor`` for one-process-per-GPU runs (registration.register(..., pairwise_executor=...),
    registration.py:2634-2655): this rank registers the pairs ``edge_owners`` assigns to it (pairs inside its brick, and its share
    of the pairs across two bricks -- a function of the whole ordered edge list, see there), then every rank receives all
    results (``gather(obj) -> list over ranks``; default: one fixed-size float64 tensor all-gather, see _gather_results)."""

    reads_only = True      # register() may hand over the images themselves instead of per-time-point copies (with a custom register_fn: set False)

    def __init__(self, rank, world_size, owners, device=0, gather=None, register_fn=None, host_threads=None):
        self.rank, self.world_size, self.owners = int(rank), int(world_size), list(owners)
        self.device, self.gather, self.register_fn, self.host_threads = device, gather, register_fn, host_threads
        if register_fn is not None:
            self.reads_only = False
        self.last_local_count = 0

    def __call__(self, msims, edges, register_kwargs):
        mine = [k for k, o in enumerate(edge_owners(edges, self.owners)) if o == self.rank]
        self.last_local_count = len(mine)
        if self.register_fn is not None:
            local = [self.register_fn(msims[edges[k][0]], msims[edges[k][1]], **register_kwargs) for k in mine]
        else:
            from . import registration

            kw = dict(register_kwargs)
            local = registration.compute_pairwise_registrations(
                msims, [edges[k] for k in mine], kw.pop("transform_key"), kw.pop("registration_binning", None),
                kw.pop("overlap_tolerance", 0.0), kw.pop("pairwise_reg_func", registration.phase_correlation_registration),
                kw.pop("pairwise_reg_func_kwargs", None), None, self.device, host_threads=self.host_threads,
                reg_res_level=kw.pop("reg_res_level", None), overlap_bbox=kw.pop("overlap_bbox", "closed_form")) if mine else []
        payload = {k: r for k, r in zip(mine, local)}
        if self.world_size == 1:
            parts = [payload]
        elif self.gather is not None:
            parts = self.gather(payload)
        else:
            parts = self._gather_results(payload, len(edges))
        results = [None] * len(edges)
        for part in parts:
            for k, r in part.items():
                results[int(k)] = r
        missing = [k for k, r in enumerate(results) if r is None]
        if missing:
            raise RuntimeError(f"no rank registered edges {missing[:8]}")
        return results


def _encode_pair_results(payload, n_edges):
    """{edge index: {"transform" (n+1, n+1), "quality", "bbox" (2, n)}} as one float64 array (n_edges, 1 + (n+1)^2 + 1 + 2n): a
    presence flag, the transform, the quality, the box; rows of edges this rank did not register are zero.  None when a result
    is not of that form (custom registration functions may return anything: those go through all_gather_object)."""
    n = None
    for r in payload.values():
        if not isinstance(r, dict) or set(r) != {"transform", "quality", "bbox"}:
            return None, None
        t, b = np.asarray(r["transform"]), np.asarray(r["bbox"])
        if t.ndim != 2 or t.shape[0] != t.shape[1] or b.shape != (2, t.shape[0] - 1) or (n is not None and t.shape[0] - 1 != n):
            return None, None
        n = t.shape[0] - 1
    if n is None:
        return None, None
    width = 1 + (n + 1) ** 2 + 1 + 2 * n
    arr = np.zeros((n_edges, width), dtype=np.float64)
    for k, r in payload.items():
        arr[k, 0] = 1.0
        arr[k, 1:1 + (n + 1) ** 2] = np.asarray(r["transform"], dtype=np.float64).reshape(-1)
        arr[k, 1 + (n + 1) ** 2] = float(r["quality"])
        arr[k, 2 + (n + 1) ** 2:] = np.asarray(r["bbox"], dtype=np.float64).reshape(-1)
    return arr, n


def _decode_pair_results(arr, n):
    out = {}
    m = (n + 1) ** 2
    for k in np.nonzero(arr[:, 0] == 1.0)[0].tolist():
        out[k] = {"transform": arr[k, 1:1 + m].reshape(n + 1, n + 1).copy(), "quality": float(arr[k, 1 + m]),
                  "bbox": arr[k, 2 + m:].reshape(2, n).copy()}
    return out


def _gather_results_impl(self, payload, n_edges):
    """Every rank's pairwise results on every rank: ONE all_gather of a fixed-size float64 tensor (kilobytes; no pickling, the
    collective the backend is good at) when the results have the standard form on every rank, all_gather_object otherwise.
    The tensor lives where the backend wants it: on this rank's GPU for nccl (RCCL), on the host for gloo."""
    import torch
    import torch.distributed as dist

    arr, n = _encode_pair_results(payload, n_edges)
    on_gpu = dist.get_backend() == "nccl"
    dev = torch.device("cuda", self.device & 0xff) if on_gpu else torch.device("cpu")
    # ranks without pairs cannot know the dimensionality, ranks with non-standard results cannot encode: agree first (one scalar)
    flag = torch.tensor([float(-1 if (payload and arr is None) else (n or 0))], dtype=torch.float64, device=dev)
    flags = [torch.zeros_like(flag) for _ in range(self.world_size)]
    dist.all_gather(flags, flag)
    dims = [int(f.item()) for f in flags]
    if any(d < 0 for d in dims) or len({d for d in dims if d > 0}) != 1:
        parts = [None] * self.world_size
        dist.all_gather_object(parts, payload)
        return parts
    n = max(dims)
    width = 1 + (n + 1) ** 2 + 1 + 2 * n
    mine = torch.from_numpy(arr if arr is not None else np.zeros((n_edges, width))).to(dev)
    bufs = [torch.zeros_like(mine) for _ in range(self.world_size)]
    dist.all_gather(bufs, mine)
    return [_decode_pair_results(b.cpu().numpy(), n) for b in bufs]


ShardedPairExecutor._gather_results = _gather_results_impl


def _fuse_sub_box(fuse_func, sims, rank, world_size, transform_key, output_stack_properties, fuse_kwargs):
    """``fuse_func`` (fusion.fuse or fusion.fuse_to_host) on ``output_stack_properties`` = rank ``rank``'s part of the global
    output stack, in the index frame of the WHOLE mosaic: every rank derives the views' parameters for the same origin and only
    shifts integer indices, so the union of the sub-boxes equals the single-GPU mosaic voxel for voxel.  Returns (result, sub-box)."""
    from . import fusion
    from . import spatial_image_utils as si_utils

    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    if output_stack_properties is None:
        output_stack_properties = fusion.process_output_stack_properties(
            list(sims), fuse_kwargs.pop("output_spacing", None), fuse_kwargs.pop("output_origin", None),
            fuse_kwargs.pop("output_shape", None), None, fuse_kwargs.pop("output_stack_mode", "union"), transform_key)
    osp = fusion._bb_dicts(output_stack_properties, sdims)
    boxes, _ = output_subboxes(osp, world_size, sdims)
    box = boxes[rank]
    sub = {k: box[k] for k in ("origin", "spacing", "shape")}
    fuse_kwargs.setdefault("frame_origin", dict(osp["origin"]))
    with warnings.catch_warnings():
        # a frame that cannot be applied would silently void the union-equals-mosaic guarantee of these functions
        warnings.simplefilter("error", fusion.IndexFrameWarning)
        fused = getattr(fusion, fuse_func)(list(sims), transform_key=transform_key, output_stack_properties=sub, **fuse_kwargs)
    return fused, box


def fuse_shard(sims, rank, world_size, transform_key, output_stack_properties=None, **fuse_kwargs):
    """Fuse this rank's sub-box of the mosaic (fusion.fuse on the rank's part of the global output stack).  Returns
    (fused sub-image, sub-box); the union over ranks is fusion.fuse of the whole mosaic."""
    return _fuse_sub_box("fuse", sims, rank, world_size, transform_key, output_stack_properties, fuse_kwargs)


def fuse_shard_to_host(sims, rank, world_size, transform_key, output_stack_properties=None, **fuse_kwargs):
    """``fuse_shard`` with the rank's sub-box ending in pinned host memory: ``fusion.fuse_to_host`` on the rank's part of the global
    output stack (z slabs of the sub-box, every slab's download under the next slab's fuse).  Returns (fused sub-image or
    (sub-image, timeline) with ``return_timeline``, sub-box)."""
    return _fuse_sub_box("fuse_to_host", sims, rank, world_size, transform_key, output_stack_properties, fuse_kwargs)


def exchange_halo(torch, dist, tiles, owners, needs, rank, world_size, device, via_host=False):
    """One-process-per-GPU halo exchange (setup, once): ``tiles[v]`` is a device tensor on the owner and None elsewhere;
    afterwards it is a tensor for every v in ``needs[rank]``.  ``needs``: list over ranks of view-index lists (every rank
    computes all of them from the metadata).  Point-to-point isend / irecv (RCCL over xGMI with the nccl backend;
    ``via_host``: staged through host tensors for backends without device support, e.g. gloo in tests).  uint16 travels as
    int16 (same bytes)."""
    def wire(t):
        t = t.view(torch.int16) if t.dtype == torch.uint16 else t
        return t.cpu() if via_host else t

    ops, recv = [], {}
    shapes = {v: (tuple(t.shape), t.dtype) for v, t in enumerate(tiles) if t is not None}
    meta = [None] * world_size
    dist.all_gather_object(meta, shapes)
    allshapes = {}
    for m in meta:
        allshapes.update(m)
    for r in range(world_size):
        for v in needs[r]:
            o = owners[v]
            if o == r:
                continue
            if rank == o:
                ops.append(dist.P2POp(dist.isend, wire(tiles[v]).contiguous(), r))
            elif rank == r:
                shp, dt = allshapes[v]
                wdt = torch.int16 if dt == torch.uint16 else dt
                recv[v] = (torch.empty(shp, dtype=wdt, device="cpu" if via_host else device), dt)
                ops.append(dist.P2POp(dist.irecv, recv[v][0], o))
    if ops:
        for w in dist.batch_isend_irecv(ops):
            w.wait()
    out = list(tiles)
    for v, (t, dt) in recv.items():
        t = t.to(device) if via_host else t
        out[v] = t.view(dt) if t.dtype != dt else t
    return out
