"""Chunk-wise fusion on the HIP backend (mirror of the reference's ``fusion`` API).

``fuse_np``  == fusion.fuse_np  (src/multiview_stitcher/fusion/_core.py:1513-1733)
``fuse``     == fusion.fuse     (_core.py:782-1501), eager, numpy- or device-backed
planner      == _build_spatial_fusion_plan and helpers (_core.py:354-722, 1736-1992)

The per-chunk arithmetic (resample + blend weights + normalise + fuse + cast)
runs as one fused kernel behind ``mvs_fuse_chunk``; this module only derives
the kernel arguments the way the reference derives scipy's.
"""

from __future__ import annotations

import collections
import contextlib
import ctypes as C
import functools
import gc
import inspect
import os
import shutil
import threading
import time
import traceback
import warnings

import numpy as np

from . import _lib, msi_utils, multiband, mv_deconv, mv_graph, ngff_utils, param_utils, streaming, weights, zarr_io
from . import device as dev_mod
from .multiband import multi_band_fusion  # noqa: F401  (fusion.multi_band_fusion)
from .mv_deconv import PSFType, multi_view_deconvolution  # noqa: F401  (fusion.multi_view_deconvolution, fusion.PSFType)
from .weights import content_based_dct  # noqa: F401  (fusion.content_based_dct)
from . import spatial_image_utils as si_utils
from .device import DeviceArray, is_device_array
from .transformation import (_as_zyx, check_interpolation_order, embed3_stack, fill_view_geometry, get_pixel_affine, get_pixel_affines,
                             shape3, transform_sim, view_data)


# --- built-in fusion / weight functions: markers dispatched to kernel modes ------------------
def weighted_average_fusion(transformed_views=None, blending_weights=None, fusion_weights=None):
    """fusion.weighted_average_fusion (_core.py:61-94) -- computed inside mvs_fuse_chunk."""
    raise RuntimeError("weighted_average_fusion is a kernel mode of mvs_fuse_chunk; pass it as fusion_func")


def max_fusion(transformed_views=None):
    """fusion.max_fusion (_core.py:42-58) -- kernel mode."""
    raise RuntimeError("max_fusion is a kernel mode of mvs_fuse_chunk; pass it as fusion_func")


def simple_average_fusion(transformed_views=None):
    """fusion.simple_average_fusion (_core.py:97-131) -- kernel mode."""
    raise RuntimeError("simple_average_fusion is a kernel mode of mvs_fuse_chunk; pass it as fusion_func")


def content_based(transformed_views=None, blending_weights=None, sigma_1=5, sigma_2=11):
    """weights.content_based (weights.py:22-74) -- kernel mode (weights_func)."""
    raise RuntimeError("content_based is a kernel mode of mvs_fuse_chunk; pass it as weights_func")


content_based.required_overlap = lambda kwargs: 2 * (kwargs or {}).get("sigma_2", 11)

_FUSION_CODES = {
    weighted_average_fusion: _lib.MVS_FUSE_WEIGHTED_AVERAGE,
    max_fusion: _lib.MVS_FUSE_MAX,
    simple_average_fusion: _lib.MVS_FUSE_SIMPLE_AVERAGE,
    "weighted_average": _lib.MVS_FUSE_WEIGHTED_AVERAGE,
    "max": _lib.MVS_FUSE_MAX,
    "simple_average": _lib.MVS_FUSE_SIMPLE_AVERAGE,
}


# The reference's own function objects (multiview_stitcher.fusion.weighted_average_fusion, ...) select the kernel
# mode of the same name: `builtin(reference_func)` is what a backend="hip" branch inside the reference would pass on
# (INTEGRATION.md section 1).
BUILTIN = {
    "weighted_average_fusion": weighted_average_fusion,
    "max_fusion": max_fusion,
    "simple_average_fusion": simple_average_fusion,
    "content_based": content_based,
    "multi_view_deconvolution": multi_view_deconvolution,   # not a kernel mode: fuse_np's deconvolution branch
    "multi_band_fusion": multi_band_fusion,                 # not a kernel mode: fuse_np's multi-band branch
    "content_based_dct": content_based_dct,                 # weights of fuse_np's mvs_fuse_chunk_dct branch
}


def builtin(func):
    """Map one of the reference's built-in fusion / weight functions (callable or name; None stays None) onto the
    kernel mode of the same name; anything else raises, custom callables cannot run inside mvs_fuse_chunk."""
    if func is None:
        return None
    name = func if isinstance(func, str) else getattr(func, "__name__", None)
    if name not in BUILTIN:
        raise NotImplementedError(f"{func!r} is not a built-in fusion/weights function of the hip backend")
    return BUILTIN[name]


def _kernel_fused(fusion_func, weights_func):
    """Fused by the kernel modes: a block is one ``mvs_fuse_chunk`` launch (a built-in fusion function, weights None or
    content_based), so the index frame, the block pipeline and -- without weights -- merged launch blocks and the replay apply."""
    return fusion_func in _FUSION_CODES and (weights_func is None or weights_func is content_based)


def _view_frames(sims, spacings, full_view_bbs):
    """``(spacings, full_view_bbs)`` of a chunk's views with the defaults filled: a slab's spacing is its whole view's, and
    without whole-view boxes every slab is a whole view."""
    if spacings is None:
        spacings = [fvb["spacing"] for fvb in full_view_bbs] if full_view_bbs is not None else [None] * len(sims)
    if full_view_bbs is None:
        full_view_bbs = [si_utils.get_stack_properties_from_sim(s) for s in sims]
    return spacings, full_view_bbs


def _trim_dict(trim_overlap_in_pixels, sdims):
    """``trim_overlap_in_pixels`` (one int, or a dict that may leave dims out) per spatial dim."""
    if not isinstance(trim_overlap_in_pixels, dict):
        return {d: int(trim_overlap_in_pixels) for d in sdims}
    return {d: int(trim_overlap_in_pixels.get(d, 0)) for d in sdims}


def _bb_dicts(bb, sdims):
    """Accept dict-of-dicts (reference) or dict-of-arrays; return dict-of-dicts keyed by sdims."""
    out = {}
    for k in ("origin", "spacing", "shape"):
        v = bb[k]
        out[k] = dict(v) if isinstance(v, dict) else dict(zip(sdims, np.asarray(v).tolist()))
    return out


def _cb_overflowed(device):
    """True when a chunk of the fast content-based path since the last check could not list the voxels its mask lacks
    (counter ``cb_overflow``: waits for the context's stream, clears the flag)."""
    return _lib.get_counter("cb_overflow", device, reset=True) > 0


@contextlib.contextmanager
def _library_option(name, device):
    """Library option ``name`` set on ``device`` for the duration.  ``cb_exact``: content-based weights through the
    bit-faithful passes; ``serial_classes``: the class kernels of a launch stay on the lane's own stream."""
    _lib.set_option(name, 1, device)
    try:
        yield
    finally:
        _lib.set_option(name, 0, device)


def fuse_np(
    sims,
    params,
    output_properties,
    fusion_func=weighted_average_fusion,
    fusion_func_kwargs=None,
    weights_func=None,
    weights_func_kwargs=None,
    trim_overlap_in_pixels=0,
    interpolation_order=1,
    full_view_bbs=None,
    spacings=None,
    origins=None,
    blending_widths=None,
    shrink_distance=0,
    backend="hip",
    output_on_backend=False,
    device=0,
    out=None,
    frame_origin=None,
    view_weights=None,
    _record=None,
    _cb_check=True,
):
    """Fuse the slabs ``sims`` of one output chunk (fusion.fuse_np, _core.py:1513-1733).

    ``sims[i]`` is a SpatialImage slab (numpy- or DeviceArray-backed, spatial dims
    only), ``params[i]`` its view->world affine, ``output_properties`` the chunk
    bounding box including halo, ``full_view_bbs[i]`` the whole view's bounding
    box (for blending weights and spacing, _core.py:1611-1646).  Returns an
    array of the chunk shape minus the trimmed halo in the input dtype; a
    ``DeviceArray`` when ``output_on_backend`` (or ``out``) is given.

    ``frame_origin`` (dict per spatial dim, optional): the INDEX FRAME of include/mvs_hip.h.  The reference derives the
    pixel offsets of every view -- and of its blend-weight support grid -- from the chunk's and the slab's origins and
    rounds them to 10 decimals (transformation.py:72-83), so two chunkings of one stack differ by ~1e-9 px in the
    weights.  With a frame origin (``fuse`` passes the output stack's) the parameters are derived once per view, for that
    origin and the WHOLE view, and the chunk / slab enter as integer index shifts: a voxel gets the same result whatever
    chunk, launch block or shard it is computed in.  Needs chunk and slab origins on the frame's grids for ALL views of the
    chunk; otherwise an ``IndexFrameWarning`` is issued and the chunk falls back to per-chunk parameters (``fuse_shard``
    turns that warning into an error: its guarantee would be lost).  Voxel-exact agreement across chunkings holds on the
    translation fast path (identity pixel matrices); the generic kernel folds ``M @ origin`` into its offsets in floating
    point, so rotated / scaled views agree across chunkings to rounding (~1e-9 px in the coordinates), not bit for bit.

    ``view_weights`` (optional): one feathered weight tile per view (``masks.feather``), or None for a view without one -- a
    uint8 sim, numpy array or ``DeviceArray`` of the view's spatial rank, always the WHOLE view's tile even where ``sims[i]`` is
    a slab.  A sim brings its own origin and spacing, in the view's own physical frame (it may live on a coarser grid, as
    ``masks.sample_masks(binning=...)`` returns it), and ``params[i]`` is applied to it whatever transforms it carries; a plain
    array has the whole view's shape and takes its origin and spacing (``full_view_bbs[i]``).  The chunk is then fused by
    ``mvs_fuse_chunk_weighted``: a view drops out where its weight is 0 and fades in with it (include/mvs_hip.h).  Built-in
    fusion functions without a ``weights_func`` only; anything else is refused by name.
    """
    if backend not in ("hip", None):
        raise ValueError("multiview_stitcher_amd.fusion.fuse_np only implements backend='hip'")
    if view_weights is not None:
        _check_view_weights_call(fusion_func, weights_func, "fuse_np")
        if len(view_weights) != len(sims):
            raise ValueError(f"view_weights: one entry per view ({len(sims)}), got {len(view_weights)}")
    check_interpolation_order(interpolation_order, "interpolation_order")
    lib = _lib.init(device)
    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    input_dtype = np.dtype(sims[0].dtype)
    if input_dtype not in _lib.DTYPE_CODES:
        raise TypeError(f"unsupported dtype {input_dtype} (uint8/uint16/float32)")
    spacings, full_view_bbs = _view_frames(sims, spacings, full_view_bbs)
    chunk = _Chunk(sims, params, sdims, _bb_dicts(output_properties, sdims), input_dtype, _trim_dict(trim_overlap_in_pixels, sdims), spacings,
                   [_bb_dicts(b, sdims) for b in full_view_bbs], int(interpolation_order), blending_widths, shrink_distance, device)
    if fusion_func is multi_view_deconvolution:
        return _fuse_np_deconvolution(chunk, fusion_func_kwargs, output_on_backend, out)
    if fusion_func is multi_band_fusion:
        if weights_func is not None:
            raise NotImplementedError("multi_band_fusion cannot be combined with a weights_func: its bands are blended by hard-seam masks")
        return _fuse_np_multiband(chunk, fusion_func_kwargs, output_on_backend, out, frame_origin)
    dct = weights_func is content_based_dct and fusion_func in _FUSION_CODES
    if dct and _FUSION_CODES[fusion_func] != _lib.MVS_FUSE_WEIGHTED_AVERAGE:
        dct, weights_func = False, None      # only a fusion_func with fusion_weights asks for them (_core.py:1665)
    elif dct:
        frame_origin, _record = None, None   # the DCT blocks are anchored at the chunk: per-chunk parameters as in the reference
    if not dct and not _kernel_fused(fusion_func, weights_func):
        # user callables (docs/extension_api_fusion.md): they run after the resample, so the chunk cannot be fused in one
        # kernel; the voxel work that is ours (resample, blending weights) still runs on the device
        return _fuse_np_with_callables(chunk, fusion_func, fusion_func_kwargs, weights_func, weights_func_kwargs, output_on_backend)
    weights_code = _lib.MVS_WEIGHTS_CONTENT_BASED if weights_func is content_based else _lib.MVS_WEIGHTS_NONE
    frame = _index_frame(chunk, frame_origin, _record)
    views, ptrs, mems, keep = _view_records(chunk, frame)
    opts, dopts = _fuse_opts(chunk, _FUSION_CODES[fusion_func], weights_code, weights_func_kwargs, frame.index_origin, dct)
    if view_weights is not None:
        wviews, tiles_alive = _weight_records(chunk, frame, view_weights)      # noqa: F841  (alive until the launch has returned)
        return _launch_chunk(lib, chunk, views, opts, dopts, out, output_on_backend, False, None, ptrs, mems, wviews=wviews)
    return _launch_chunk(lib, chunk, views, opts, dopts, out, output_on_backend, weights_code and _cb_check, _record, ptrs, mems)


def _check_view_weights_call(fusion_func, weights_func, who):
    """``view_weights`` go with the kernel modes without a ``weights_func``; every other combination is refused by name."""
    if weights_func is not None:
        raise NotImplementedError(f"{who}: view_weights cannot be combined with a weights_func "
                                  f"({getattr(weights_func, '__name__', weights_func)!r}): the weighted chunk kernel has no content-based weights")
    if fusion_func is multi_view_deconvolution:
        raise NotImplementedError(f"{who}: view_weights cannot be combined with multi_view_deconvolution")
    if fusion_func is multi_band_fusion:
        raise NotImplementedError(f"{who}: view_weights cannot be combined with multi_band_fusion: its bands are blended by hard-seam masks")
    if fusion_func not in _FUSION_CODES:
        raise NotImplementedError(f"{who}: view_weights cannot be combined with the user callable {getattr(fusion_func, '__name__', fusion_func)!r}; "
                                  "they go with weighted_average_fusion, max_fusion and simple_average_fusion")


def _weight_tile(entry, view_bb, sdims, who, i):
    """``(data, origin, spacing)`` of the weight tile of view ``i``: a sim's own coordinates, or the whole view's for a plain array
    of its shape.  ``t`` / ``c`` dims (per-time-point weight tiles) are refused by name."""
    if isinstance(entry, si_utils.SpatialImage) or msi_utils.is_msim(entry):
        sim = msi_utils.get_sim_from_msim(entry, scale="scale0") if msi_utils.is_msim(entry) else entry
        for d in sim.dims:
            if d in ("t", "c"):
                raise NotImplementedError(f"{who}: view_weights[{i}] has a {d!r} dim; per-time-point / per-channel weight tiles are not supported "
                                          "(one spatial tile per view)")
        if list(si_utils.get_spatial_dims_from_sim(sim)) != list(sdims):
            raise ValueError(f"{who}: view_weights[{i}] has dims {list(sim.dims)}, the view {list(sdims)}")
        data, origin, spacing = sim.data, si_utils.get_origin_from_sim(sim, asarray=True), si_utils.get_spacing_from_sim(sim, asarray=True)
    else:
        data = entry if is_device_array(entry) else np.asarray(entry)
        if tuple(int(n) for n in data.shape) != tuple(int(view_bb["shape"][d]) for d in sdims):
            raise ValueError(f"{who}: view_weights[{i}] has shape {tuple(data.shape)}, the view {tuple(int(view_bb['shape'][d]) for d in sdims)}; "
                             "a tile on another grid comes as a sim with its own coordinates")
        origin, spacing = _as_zyx(view_bb["origin"], sdims), _as_zyx(view_bb["spacing"], sdims)
    if np.dtype(data.dtype) != np.uint8:
        raise TypeError(f"{who}: view_weights[{i}] is {data.dtype}; weight tiles are uint8 (masks.feather)")
    return data, origin, spacing


def _weight_records(chunk, frame, view_weights):
    """The ``mvs_view_t`` array of the chunk's weight tiles (``data`` NULL where a view has none) and what keeps their memory alive.
    The pixel affines are derived as ``_view_records`` derives the images': for the frame's origin, the chunk entering as an
    integer index shift; a tile is whole, so its own index offset is 0."""
    sdims, n = chunk.sdims, len(chunk.sims)
    wviews = (_lib.mvs_view_t * n)()
    keep = []
    out_spacing = _as_zyx(chunk.out_bb["spacing"], sdims)
    for i, entry in enumerate(view_weights):
        if entry is None:
            continue
        data, origin, spacing = _weight_tile(entry, chunk.full_view_bbs[i], sdims, "fuse_np", i)
        p_inv = np.linalg.inv(np.asarray(chunk.params[i], dtype=np.float64))
        matrices, offsets = get_pixel_affines(p_inv[None], origin[None], spacing[None], frame.out_origin, out_spacing)
        ptr, s3, st3, mem, kept = view_data(data, chunk.device, np.dtype(np.uint8))
        fill_view_geometry(wviews[i], ptr, _lib.MVS_U8, mem, s3, st3, matrices[0], offsets[0])
        keep.append(kept)
    return wviews, keep


# One fuse_np call with its arguments normalised, as the three forms (kernel modes, deconvolution, callables) receive it:
# ``out_bb`` the chunk box incl. halo as dict-of-dicts, ``trim`` the halo to cut per spatial dim, ``spacings`` a slab's spacing or
# None (= read it from the slab), ``full_view_bbs`` the whole views' boxes as dict-of-dicts (see ``_view_frames``).
_Chunk = collections.namedtuple(
    "_Chunk", "sims params sdims out_bb input_dtype trim spacings full_view_bbs order blending_widths shrink_distance device")

# The index frame of one chunk (``_index_frame``): integer shifts of the chunk (``index_origin``, 3) and of every slab
# (``index_offsets``, (n, 3)) against the origins the parameters are derived for (``out_origin``; ``in_origins`` per view); next
# to them the stacked per-view geometry they were computed from.
_Frame = collections.namedtuple("_Frame", "index_origin index_offsets out_origin in_origins in_spacings full_origins")


def _index_frame(chunk, frame_origin, record):
    """Chunk and slabs as integer index shifts of parameters derived for (frame origin, whole view) -- or, without a
    ``frame_origin`` or with one that does not apply (an origin off the frame's grids: ``IndexFrameWarning``, attributed to
    fuse_np's caller), no shifts and the chunk's and slabs' own origins."""
    sdims, ndim, n = chunk.sdims, len(chunk.sdims), len(chunk.sims)
    out_origin, out_spacing = _as_zyx(chunk.out_bb["origin"], sdims), _as_zyx(chunk.out_bb["spacing"], sdims)
    in_spacings = np.stack([_as_zyx(sp if sp is not None else si_utils.get_spacing_from_sim(sim), sdims)
                            for sim, sp in zip(chunk.sims, chunk.spacings)])
    in_origins = np.stack([si_utils.get_origin_from_sim(sim, asarray=True) for sim in chunk.sims])
    full_origins = np.stack([_as_zyx(b["origin"], sdims) for b in chunk.full_view_bbs])
    index_origin, index_offsets = np.zeros(3, np.int64), np.zeros((n, 3), np.int64)
    if frame_origin is not None:
        f_origin = _as_zyx(frame_origin, sdims)
        io_ = (out_origin - f_origin) / out_spacing
        so_ = (in_origins - full_origins) / in_spacings
        if np.all(np.abs(io_ - np.round(io_)) < 1e-6) and np.all(np.abs(so_ - np.round(so_)) < 1e-6):
            index_origin[3 - ndim:] = np.round(io_).astype(np.int64)
            index_offsets[:, 3 - ndim:] = np.round(so_).astype(np.int64)
            return _Frame(index_origin, index_offsets, f_origin, full_origins, in_spacings, full_origins)
        off_c = float(np.abs(io_ - np.round(io_)).max()) if io_.size else 0.0
        off_s = float(np.abs(so_ - np.round(so_)).max()) if so_.size else 0.0      # (a chunk without views has no slabs)
        warnings.warn(
            "fuse_np: frame_origin cannot be applied -- the chunk origin or a slab origin is not on the frame's grid "
            f"(largest distance from it: chunk {off_c:.3g} px, slabs {off_s:.3g} px); the parameters of this chunk are derived per chunk, so its "
            "voxels may differ in the last bit from the same voxels fused through another chunk, launch block or shard",
            IndexFrameWarning, stacklevel=3)
        if record is not None:
            record["no_replay"] = True      # (a replayed call would not repeat the warning)
    return _Frame(index_origin, index_offsets, out_origin, in_origins, in_spacings, full_origins)


def _view_records(chunk, frame):
    """The ``mvs_view_t`` array of a chunk: ``(views, data pointers, memory codes, keep-alive list)``."""
    sdims, device, n = chunk.sdims, chunk.device, len(chunk.sims)
    views = (_lib.mvs_view_t * n)()
    keep = []
    # the view records are computed for all views at once (stacked arrays: the per-view form of the same arithmetic costs
    # ~70 us of interpreter time per view) and written into the ctypes array through a byte view
    p_inv = np.linalg.inv(np.stack([np.asarray(p, dtype=np.float64) for p in chunk.params]))
    out_spacing = _as_zyx(chunk.out_bb["spacing"], sdims)
    matrices, offsets = get_pixel_affines(p_inv, frame.in_origins, frame.in_spacings, frame.out_origin, out_spacing)
    tables, sup_origins, sup_spacings = weights.blending_supports(
        frame.full_origins, np.stack([_as_zyx(b["spacing"], sdims) for b in chunk.full_view_bbs]),
        np.stack([_as_zyx(b["shape"], sdims) for b in chunk.full_view_bbs]), sdims, chunk.blending_widths, chunk.shrink_distance)
    w_matrices, w_offsets = get_pixel_affines(p_inv, sup_origins, sup_spacings, frame.out_origin, out_spacing)
    ptrs, mems, shapes, strides = np.zeros(n, np.uint64), np.zeros(n, np.int32), np.ones((n, 3), np.int64), np.zeros((n, 3), np.int64)
    for i, sim in enumerate(chunk.sims):
        ptrs[i], shapes[i], strides[i], mems[i], data = view_data(sim.data, device, chunk.input_dtype)
        keep.append(data)
    V = _lib.mvs_view_t
    rec = np.frombuffer(views, dtype=np.uint8).reshape(n, C.sizeof(V))

    def field(name, dtype, count):
        off = getattr(V, name).offset
        return rec[:, off:off + count * np.dtype(dtype).itemsize].view(dtype)

    m3, o3 = embed3_stack(matrices, offsets)
    wm3, wo3 = embed3_stack(w_matrices, w_offsets)
    field("data", np.uint64, 1)[:, 0] = ptrs
    field("dtype", np.int32, 1)[:, 0] = _lib.DTYPE_CODES[chunk.input_dtype]
    field("mem", np.int32, 1)[:, 0] = mems
    field("shape", np.int64, 3)[:] = shapes
    field("stride", np.int64, 3)[:] = strides
    field("matrix", np.float64, 9)[:] = m3
    field("offset", np.float64, 3)[:] = o3
    field("w_matrix", np.float64, 9)[:] = wm3
    field("w_offset", np.float64, 3)[:] = wo3
    field("index_offset", np.int64, 3)[:] = frame.index_offsets
    edt = field("edt", np.float32, 125)
    edt[:] = 0
    for i, table in enumerate(tables):
        edt[i, : table.size] = table.reshape(-1)
    return views, ptrs, mems, keep


def _fuse_opts(chunk, fusion_code, weights_code, weights_func_kwargs, index_origin, dct):
    """The ``mvs_fuse_opts_t`` of a chunk (``out_mem`` is set by the launch) and, with ``dct``, its ``mvs_dct_opts_t``."""
    sdims, ndim = chunk.sdims, len(chunk.sdims)
    opts = _lib.mvs_fuse_opts_t()
    opts.ndim = ndim
    opts.order = chunk.order
    opts.fusion = fusion_code
    opts.weights = weights_code
    s3, t3 = shape3([int(chunk.out_bb["shape"][d]) for d in sdims]), [0] * (3 - ndim) + [chunk.trim[d] for d in sdims]
    for k in range(3):
        opts.out_shape[k] = s3[k]
        opts.trim[k] = t3[k]
        opts.index_origin[k] = int(index_origin[k])
    wk = weights_func_kwargs or {}
    opts.sigma_1 = float(wk.get("sigma_1", 5))
    opts.sigma_2 = float(wk.get("sigma_2", 11))
    opts.out_dtype = _lib.DTYPE_CODES[chunk.input_dtype]
    if not dct:
        return opts, None
    # content_based_dct's arguments as the reference passes them (_core.py:1665-1682): output_chunksize defaults to the
    # chunk's shape including the halo
    dkw = dict(wk)
    for k in ("transformed_views", "device"):
        if k in dkw:
            raise TypeError(f"weights_func_kwargs must not set {k!r}: fuse_np supplies it")
    if dkw.get("output_chunksize") is None:
        dkw["output_chunksize"] = dict(chunk.out_bb["shape"])
    return opts, weights.dct_opts(ndim, **dkw)


def _launch_chunk(lib, chunk, views, opts, dopts, out, output_on_backend, cb_check, record, ptrs, mems, wviews=None):
    """One ``mvs_fuse_chunk`` (``mvs_fuse_chunk_dct`` with ``dopts``, ``mvs_fuse_chunk_weighted`` with ``wviews``) launch into
    ``out`` / a new device array / a new host array.  ``cb_check``: a content-based result left on the device is checked for a
    mask-list overflow.  ``record``: where fuse()'s geometry-keyed replay remembers a launch whose views are all resident on the
    device (``mems``), or None."""
    device, n = chunk.device, len(views)
    res_shape = [int(chunk.out_bb["shape"][d]) - 2 * chunk.trim[d] for d in chunk.sdims]

    def launch(dst):
        if wviews is not None:
            return lib.mvs_fuse_chunk_weighted(device, views, wviews, n, C.byref(opts), dst), "mvs_fuse_chunk_weighted"
        if dopts is not None:
            return lib.mvs_fuse_chunk_dct(device, views, n, C.byref(opts), C.byref(dopts), dst), "mvs_fuse_chunk_dct"
        return lib.mvs_fuse_chunk(device, views, n, C.byref(opts), dst), "mvs_fuse_chunk"

    if out is not None or output_on_backend:
        if out is None:
            out = DeviceArray.empty(res_shape, chunk.input_dtype, device)
        if tuple(out.shape) != tuple(res_shape) or not out.is_contiguous():
            raise ValueError("out must be a contiguous DeviceArray of the result shape")
        opts.out_mem = _lib.MVS_MEM_DEVICE
        rc, what = launch(C.c_void_p(out.ptr))
        _lib.check(rc, device, what)
        if cb_check and _cb_overflowed(device):
            # the fast content-based path lists the voxels its box-shaped mask lacks; a list that did not fit raised a flag
            # (a result left on the device is not waited for inside the call): this chunk again through the bit-faithful passes
            with _library_option("cb_exact", device):
                rc = lib.mvs_fuse_chunk(device, views, n, C.byref(opts), C.c_void_p(out.ptr))
                _lib.check(rc, device, "mvs_fuse_chunk")
        out.mark_written()
        if record is not None and bool(np.all(mems == _lib.MVS_MEM_DEVICE)):
            # (the view records without their data pointers, the options, the result shape)
            record.update(views=bytes(views), opts=bytes(opts), n=n, res_shape=tuple(int(v) for v in res_shape), ptrs=ptrs.copy())
        return out
    result = np.empty(tuple(res_shape), dtype=chunk.input_dtype)
    opts.out_mem = _lib.MVS_MEM_HOST
    rc, what = launch(result.ctypes.data)
    _lib.check(rc, device, what)
    return result


def _resampled_stacks(chunk, weights_frame=None):
    """The prologue the stack-based fusion functions share (_core.py:1608-1649): every view of the chunk resampled by mvs_resample
    (float32, NaN outside) and its raw blending weights by mvs_blend_weights, as two device stacks (V, *S).  The parameters are
    derived per chunk, as the reference does.  ``weights_frame`` = (frame origin (zyx array), index_origin (3 ints)): the blending
    weights are derived for the frame's grid instead and the chunk enters as an integer index shift (mvs_blend_weights_at), so a
    voxel's weights have the same bits in every chunk of the frame."""
    sims, params, sdims, out_bb, device = chunk.sims, chunk.params, chunk.sdims, chunk.out_bb, chunk.device
    lib = _lib.init(device)
    ndim, n = len(sdims), len(sims)
    out_shape = tuple(int(out_bb["shape"][d]) for d in sdims)
    o_origin, o_spacing = _as_zyx(out_bb["origin"], sdims), _as_zyx(out_bb["spacing"], sdims)
    S = int(np.prod(out_shape))
    views_t = DeviceArray.empty((n,) + out_shape, np.float32, device)
    blend = DeviceArray.empty((n,) + out_shape, np.float32, device)
    s3 = _lib.i64x3(shape3(out_shape))
    keep = []
    for i, (sim, param, spacing) in enumerate(zip(sims, params, chunk.spacings)):
        p_inv = np.linalg.inv(np.asarray(param, dtype=np.float64))
        in_spacing = spacing if spacing is not None else si_utils.get_spacing_from_sim(sim)
        matrix, offset = get_pixel_affine(p_inv, si_utils.get_origin_from_sim(sim, asarray=True), _as_zyx(in_spacing, sdims),
                                          o_origin, o_spacing)
        view = _lib.mvs_view_t()
        ptr, shape, strides, mem, data = view_data(sim.data, device)
        fill_view_geometry(view, ptr, _lib.DTYPE_CODES[data.dtype], mem, shape, strides, matrix, offset)
        keep.append(data)
        rc = lib.mvs_resample(device, C.byref(view), s3, chunk.order, float("nan"), C.c_void_p(views_t.ptr + 4 * i * S),
                              _lib.MVS_MEM_DEVICE)
        _lib.check(rc, device, "mvs_resample")
        wview = _lib.mvs_view_t()
        weights.fill_view_weights(wview, chunk.full_view_bbs[i], param, o_origin if weights_frame is None else weights_frame[0], o_spacing,
                                  chunk.blending_widths, chunk.shrink_distance)
        if weights_frame is None:
            rc = lib.mvs_blend_weights(device, C.byref(wview), ndim, s3, C.c_void_p(blend.ptr + 4 * i * S), _lib.MVS_MEM_DEVICE)
        else:
            rc = lib.mvs_blend_weights_at(device, C.byref(wview), ndim, s3, _lib.i64x3(weights_frame[1]), C.c_void_p(blend.ptr + 4 * i * S),
                                          _lib.MVS_MEM_DEVICE)
        _lib.check(rc, device, "mvs_blend_weights")
    return views_t, blend


def _supplied_kwargs(fusion_func_kwargs):
    """A copy of ``fusion_func_kwargs`` without the arguments fuse_np supplies itself (setting one is a ``TypeError``)."""
    kw = dict(fusion_func_kwargs or {})
    for k in ("transformed_views", "blending_weights", "device"):
        if k in kw:
            raise TypeError(f"fusion_func_kwargs must not set {k!r}: fuse_np supplies it")
    return kw


def _fuse_np_deconvolution(chunk, fusion_func_kwargs, output_on_backend, out):
    """fuse_np with ``fusion_func=multi_view_deconvolution`` (_core.py:1608-1713 around mv_deconv.py:251-501), all on the
    device: every view resampled by mvs_resample (float32, NaN outside) and its blending weights by mvs_blend_weights
    into two (V, *S) stacks; mvs_mv_deconv masks the weights by ~isnan and normalises them, deconvolves, trims the halo,
    applies nan_to_num and casts to the input dtype.  ``output_spacing`` is the chunk spacing unless the caller passed
    one (_core.py:1658-1662).  Only the result crosses PCIe, and only when a host result is asked for."""
    ndim = len(chunk.sdims)
    kw = _supplied_kwargs(fusion_func_kwargs)
    if kw.get("output_spacing") is None:
        kw["output_spacing"] = dict(chunk.out_bb["spacing"])
    kernels = mv_deconv._kernels(len(chunk.sims), ndim, kw.get("psfs"), kw.get("psf_type", PSFType.EFFICIENT_BAYESIAN), kw["output_spacing"],
                                 kw.get("na", 0.8), kw.get("wavelength_um", 0.5))
    views_t, blend = _resampled_stacks(chunk)
    trim = list(chunk.trim.values())
    on_device = out is not None or output_on_backend
    res = mv_deconv._run(views_t, blend, ndim, kernels, kw.get("n_iterations", 10), kw.get("lambda_reg", 0.0),
                         kw.get("min_value", 1e-4), kw.get("sample_boundary_erosion_px", 0), trim, chunk.input_dtype, on_device, chunk.device,
                         prepare_weights=True, out=out)
    return res


def _fuse_np_multiband(chunk, fusion_func_kwargs, output_on_backend, out, frame_origin):
    """fuse_np with ``fusion_func=multi_band_fusion``, all on the device: the stacks of ``_resampled_stacks``, then ONE
    mvs_multiband_fuse call (masking, pyramids, blend, collapse, halo trim, cast to the input dtype).  The pyramids decimate on the
    lattice of ``frame_origin``: ``index_origin = (chunk origin - frame origin) / spacing``; an origin off that grid (not within 1e-6 of
    integers) issues an ``IndexFrameWarning`` and the chunk is anchored at 0.  Only the result crosses PCIe, and only when a host
    result is asked for."""
    sdims, ndim = chunk.sdims, len(chunk.sdims)
    kw = _supplied_kwargs(fusion_func_kwargs)
    unknown = sorted(set(kw) - {"n_levels", "index_origin"})
    if unknown:
        raise TypeError(f"multi_band_fusion got unexpected fusion_func_kwargs {unknown}")
    if "index_origin" in kw:
        raise TypeError("fusion_func_kwargs must not set 'index_origin': fuse_np derives it from frame_origin")
    levels3 = multiband._levels3(kw.get("n_levels", 3), ndim)
    origin3, weights_frame = [0, 0, 0], None
    if frame_origin is not None:
        io_ = (_as_zyx(chunk.out_bb["origin"], sdims) - _as_zyx(frame_origin, sdims)) / _as_zyx(chunk.out_bb["spacing"], sdims)
        if np.all(np.abs(io_ - np.round(io_)) < 1e-6):
            origin3[3 - ndim:] = [int(v) for v in np.round(io_)]
            # the winner map compares the weights themselves: they are derived once for the frame, the chunk is an index shift
            weights_frame = (_as_zyx(frame_origin, sdims), origin3)
        else:
            warnings.warn(
                "fuse_np: frame_origin cannot be applied -- the chunk origin is not on the frame's grid (largest distance from it: "
                f"{float(np.abs(io_ - np.round(io_)).max()):.3g} px); the pyramids of this chunk are anchored at its own first sample, so its "
                "voxels may differ from the same voxels fused through another chunk", IndexFrameWarning, stacklevel=3)
    views_t, blend = _resampled_stacks(chunk, weights_frame)
    on_device = out is not None or output_on_backend
    return multiband._run(views_t, blend, ndim, levels3, origin3, list(chunk.trim.values()), chunk.input_dtype, on_device, chunk.device, out=out)


def _host_weighted_average_fusion(transformed_views, blending_weights, fusion_weights=None):
    """weighted_average_fusion on host arrays (_core.py:61-94) -- used when a custom weights_func supplies fusion_weights."""
    if fusion_weights is None:
        additive = blending_weights
    else:
        additive = blending_weights * fusion_weights
        wsum = np.nansum(additive, axis=0)            # weights.normalize_weights (weights.py:325-345)
        wsum[wsum == 0] = 1
        additive = additive / wsum
    return np.nansum(transformed_views * additive, axis=0).astype(transformed_views[0].dtype)


def _host_max_fusion(transformed_views):
    """max_fusion on host arrays (_core.py:42-58)."""
    return np.nanmax(transformed_views, axis=0)


def _host_simple_average_fusion(transformed_views):
    """simple_average_fusion on host arrays (_core.py:97-131)."""
    nvalid = np.sum(~np.isnan(transformed_views), axis=0).astype(np.float32)
    nvalid[nvalid == 0] = np.nan
    return (np.nansum(transformed_views, axis=0) / nvalid).astype(transformed_views[0].dtype)


_HOST_FUSION = {weighted_average_fusion: _host_weighted_average_fusion, max_fusion: _host_max_fusion,
                simple_average_fusion: _host_simple_average_fusion}


def has_keyword(func, keyword):
    """misc_utils.has_keyword (misc_utils.py:69-80): does ``func`` accept ``keyword``?"""
    try:
        return keyword in inspect.signature(func).parameters
    except (TypeError, ValueError):
        return False


def _fuse_np_with_callables(chunk, fusion_func, fusion_func_kwargs, weights_func, weights_func_kwargs, output_on_backend):
    """fuse_np for user-supplied ``fusion_func`` / ``weights_func`` callables (_core.py:1608-1733): every view is
    resampled with mvs_resample (float32, NaN outside), blending weights come from mvs_blend_weights and are
    normalised like weights.normalize_weights (weights.py:325-345); the callables then receive host float32
    arrays exactly as in the reference (``transformed_views`` (V, *S), ``blending_weights``, ``fusion_weights``,
    ``params``, ``output_spacing`` / ``output_chunksize`` when they ask for them)."""
    sims, params, sdims, out_bb, device = chunk.sims, chunk.params, chunk.sdims, chunk.out_bb, chunk.device
    # A custom weights_func with one of the built-in fusion functions (the documented extension case, _core.py:1663-1690):
    # the built-ins are kernel modes here, so their host form takes over behind the user's weights.
    fusion_func = _HOST_FUSION.get(fusion_func, fusion_func) if not isinstance(fusion_func, str) else _HOST_FUSION[BUILTIN[fusion_func + "_fusion"]]
    fusion_func_kwargs = dict(fusion_func_kwargs or {})
    weights_func_kwargs = dict(weights_func_kwargs or {})

    def host(a):
        return a.get() if is_device_array(a) else np.asarray(a)

    views_t = np.stack([
        host(transform_sim(sim, np.linalg.inv(np.asarray(param, dtype=np.float64)), output_stack_properties=out_bb,
                           input_spacing=spacing, order=chunk.order, cval=np.nan, device=device,
                           allow_noop=False).data).astype(np.float32, copy=False)
        for sim, param, spacing in zip(sims, params, chunk.spacings)
    ])
    needs_blending = has_keyword(fusion_func, "blending_weights") or (
        weights_func is not None and has_keyword(weights_func, "blending_weights"))
    blend = None
    if needs_blending:
        blend = np.stack([
            weights.get_blending_weights(out_bb, chunk.full_view_bbs[i], params[i], chunk.blending_widths, chunk.shrink_distance, device)
            for i in range(len(sims))
        ])
        blend = blend * ~np.isnan(views_t)
        wsum = np.nansum(blend, axis=0)
        wsum[wsum == 0] = 1
        blend = blend / wsum
    fusion_func_kwargs["transformed_views"] = views_t
    if has_keyword(fusion_func, "params"):
        fusion_func_kwargs["params"] = params
    if has_keyword(fusion_func, "blending_weights"):
        fusion_func_kwargs["blending_weights"] = blend
    if has_keyword(fusion_func, "output_spacing") and "output_spacing" not in fusion_func_kwargs:
        fusion_func_kwargs["output_spacing"] = out_bb["spacing"]
    if weights_func is not None and has_keyword(fusion_func, "fusion_weights"):
        if weights_func is content_based:
            raise NotImplementedError("content_based weights with a custom fusion_func: pass a callable weights_func")
        weights_func_kwargs["transformed_views"] = views_t
        if has_keyword(weights_func, "params"):
            weights_func_kwargs["params"] = params
        if has_keyword(weights_func, "blending_weights"):
            weights_func_kwargs["blending_weights"] = blend
        if has_keyword(weights_func, "output_chunksize") and "output_chunksize" not in weights_func_kwargs:
            weights_func_kwargs["output_chunksize"] = out_bb["shape"]
        fusion_func_kwargs["fusion_weights"] = weights_func(**weights_func_kwargs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)   # func_ignore_nan_warning (_core.py:1684-1687)
        fused = np.asarray(fusion_func(**fusion_func_kwargs))
    trim = chunk.trim
    if any(trim[d] > 0 for d in sdims):
        fused = fused[tuple(slice(trim[d], -trim[d]) if trim[d] > 0 else slice(None) for d in sdims)]
    fused = np.nan_to_num(fused).astype(chunk.input_dtype)
    if output_on_backend:
        return DeviceArray.from_host(np.ascontiguousarray(fused), device)
    return fused


# --- output stack properties (_core.py:1736-1992) ---------------------------------------------
def calc_stack_properties_from_volume(volume, spacing):
    """_core.py:1972-1992: shape = floor(extent/spacing + 1e-9) + 1."""
    origin = volume[0]
    shape = np.floor((volume[1] - volume[0]) / spacing + 1e-9).astype(np.uint64) + 1
    return {"shape": shape, "spacing": spacing, "origin": origin}


def get_transformed_stack_vertices(stack_keypoints, stack_properties_list, params):
    """_core.py:1947-1969."""
    ndim = len(stack_properties_list[0]["spacing"])
    vertices = np.zeros((len(stack_properties_list), len(stack_keypoints), ndim))
    for iim, sp in enumerate(stack_properties_list):
        tmp = stack_keypoints * (np.array(sp["shape"]) - 1) * np.array(sp["spacing"]) + np.array(sp["origin"])
        vertices[iim] = np.dot(params[iim][:ndim, :ndim], tmp.T).T + params[iim][:ndim, ndim]
    return vertices


def calc_stack_properties_from_view_properties_and_params(views_props, params, spacing, mode="union"):
    """_core.py:1821-1899 (modes union / intersection / sample)."""
    sdims = ["z", "y", "x"][-len(spacing):]
    spacing = np.array([spacing[d] for d in sdims]).astype(float)
    views_props = [{k: np.array([v[d] for d in sdims]) for k, v in vp.items()} for vp in views_props]
    ndim = len(spacing)
    stack_vertices = np.array(list(np.ndindex(tuple([2] * ndim)))).astype(float)
    if mode == "sample":
        zface = stack_vertices[np.where(stack_vertices[:, 0] == 1)]
        zface[:, 2] = np.mean(zface[:, 2])
        tv = get_transformed_stack_vertices(zface, views_props, params)
        volume = np.min(np.min(tv, 1), 0), np.max(np.max(tv, 1), 0)
    elif mode == "union":
        tv = get_transformed_stack_vertices(stack_vertices, views_props, params)
        volume = np.min(np.min(tv, 1), 0), np.max(np.max(tv, 1), 0)
    elif mode == "intersection":
        tv = get_transformed_stack_vertices(stack_vertices, views_props, params)
        volume = np.max(np.min(tv, 1), 0), np.min(np.max(tv, 1), 0)
    else:
        raise ValueError(f"unknown output_stack_mode {mode!r}")
    return calc_stack_properties_from_volume(volume, spacing)


def combine_stack_props(stack_props_list):
    """_core.py:1902-1944."""
    origin = np.min([sp["origin"] for sp in stack_props_list], axis=0)
    spacing = np.min([sp["spacing"] for sp in stack_props_list], axis=0)
    shape = (
        np.max(
            [np.floor((sp["origin"] + (sp["shape"] - 1) * sp["spacing"] - origin) / spacing + 1e-9) for sp in stack_props_list],
            axis=0,
        ).astype(np.uint64)
        + 1
    )
    return {"origin": origin, "spacing": spacing, "shape": shape}


def calc_fusion_stack_properties(sims, params, spacing, mode="union"):
    """fusion.calc_fusion_stack_properties (_core.py:1736-1818); params may be t-stacked."""
    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    views_props = [si_utils.get_stack_properties_from_sim(sim) for sim in sims]
    params = [np.asarray(p, dtype=np.float64) for p in params]
    nt = max([p.shape[0] for p in params if p.ndim == 3] + [0])
    if nt:
        sp = combine_stack_props(
            [
                calc_stack_properties_from_view_properties_and_params(
                    views_props, [param_utils.select_time(p, it) for p in params], spacing, mode
                )
                for it in range(nt)
            ]
        )
    else:
        sp = calc_stack_properties_from_view_properties_and_params(views_props, params, spacing, mode)
    return {k: {d: (int(v[i]) if k == "shape" else float(v[i])) for i, d in enumerate(sdims)} for k, v in sp.items()}


def process_output_stack_properties(
    sims, output_spacing=None, output_origin=None, output_shape=None, output_stack_properties=None,
    output_stack_mode="union", transform_key=None,
):
    """_core.py:296-333."""
    if transform_key is None:
        raise ValueError("transform_key must be provided to determine transformation parameters")
    params = [si_utils.get_affine_from_sim(sim, transform_key) for sim in sims]
    if output_stack_properties is None:
        if output_spacing is None:
            output_spacing = si_utils.get_spacing_from_sim(sims[0])
        output_stack_properties = calc_fusion_stack_properties(sims, params, output_spacing, output_stack_mode)
        if output_origin is not None:
            output_stack_properties["origin"] = output_origin
        if output_shape is not None:
            output_stack_properties["shape"] = output_shape
    return output_stack_properties


def process_output_chunksize(sims, output_chunksize):
    """_core.py:248-277 (numpy-backed tiles -> the spatial_image_utils defaults)."""
    ndim = si_utils.get_ndim_from_sim(sims[0])
    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    if output_chunksize is None:
        output_chunksize = si_utils.get_default_spatial_chunksizes(ndim)
    elif isinstance(output_chunksize, int):
        output_chunksize = {dim: output_chunksize for dim in sdims}
    return output_chunksize


MAX_LAUNCH_BYTES = int(os.environ.get("MVS_MAX_LAUNCH_BYTES", 32 << 30))
MAX_STREAM_BYTES = int(os.environ.get("MVS_MAX_STREAM_BYTES", 1 << 30))      # launch block of a fuse() that reads or writes Zarr stores


def _merged_chunksize(chunksize, shape, sdims, itemsize, max_bytes=None):
    """Launch-block size for fuse(merge_chunks=True): whole multiples of the requested chunk size, as large as fits
    ``max_bytes`` of output -- the whole stack if possible, otherwise the block count is doubled along the axis with
    the longest blocks (first axis on ties) until a block fits."""
    max_bytes = MAX_LAUNCH_BYTES if max_bytes is None else int(max_bytes)
    cs = {d: max(int(chunksize[d]), 1) for d in sdims}
    nchunks = {d: -(-int(shape[d]) // cs[d]) for d in sdims}
    parts = {d: 1 for d in sdims}

    def block(d):
        return min(-(-nchunks[d] // parts[d]) * cs[d], int(shape[d]))

    while int(np.prod([block(d) for d in sdims])) * itemsize > max_bytes:
        cand = [d for d in sdims if parts[d] < nchunks[d]]
        if not cand:
            break
        d = max(cand, key=lambda d_: block(d_))
        parts[d] = min(parts[d] * 2, nchunks[d])
    return {d: block(d) for d in sdims}


def _launch_budget(sims, out_shape, sdims, itemsize, device, cap, view_weights=None):
    """Output bytes one launch block of fuse(merge_chunks=True) may take so that the launch fits the device: the block
    itself plus the view slabs that have to be STAGED for it (host- or Zarr-backed views, and views resident on another
    GPU, are copied into device scratch; views already on ``device`` cost nothing) must stay below 90 % of the free
    device memory (``mvs_mem_info``).  The staged share is estimated per output byte: twice the mosaic-average (overlap
    zones hold every voxel two to eight times) plus one whole view.  ``view_weights``: the weight tiles of the call stay resident
    for all its blocks, so those that still have to be uploaded come off the free memory first.  Never above ``cap``
    (MVS_MAX_LAUNCH_BYTES / MVS_MAX_STREAM_BYTES)."""
    try:
        free, _ = _lib.mem_info(device)
    except (RuntimeError, OSError, AttributeError):
        return cap
    staged, largest = 0, 0
    for s in sims:
        data = s.data
        if is_device_array(data) and (data.device & 0xff) == (int(device) & 0xff):
            continue
        nb = int(np.prod([s.sizes[d] for d in sdims])) * itemsize
        staged += nb
        largest = max(largest, nb)
    out_total = max(int(np.prod([int(out_shape[d]) for d in sdims])) * itemsize, 1)
    avail = int(0.9 * free) - largest - _weight_upload_bytes(view_weights, device)
    per_out_byte = 1.0 + 2.0 * staged / out_total
    return int(max(min(cap, avail / per_out_byte), 1))


def _weight_data(entry):
    """The array of a ``view_weights`` entry (a sim's data, or the entry itself)."""
    if msi_utils.is_msim(entry):
        entry = msi_utils.get_sim_from_msim(entry, scale="scale0")
    return entry.data if isinstance(entry, si_utils.SpatialImage) else entry


def _weight_upload_bytes(view_weights, device):
    """Bytes of the weight tiles that are not yet resident on ``device`` (uint8: one byte per voxel)."""
    total = 0
    for entry in view_weights or ():
        data = None if entry is None else _weight_data(entry)
        if data is not None and not (is_device_array(data) and (data.device & 0xff) == (int(device) & 0xff)):
            total += int(np.prod(data.shape))
    return total


def _resident_weight(data, device):
    """A weight tile as a ``DeviceArray``: itself, or uploaded to ``device`` (once per fuse() call, what ``device.to_device`` does
    for a view)."""
    return data if is_device_array(data) else DeviceArray.from_host(np.ascontiguousarray(data), device)


def _upload_view_weights(call):
    """``dev_weights``: per view its weight tile resident on the device -- a sim keeps its coordinates, a plain array stays an array
    -- or None.  Every tile is checked against its view first (``_weight_tile``), so a wrong entry fails before any block is fused."""
    call.dev_weights = None
    if call.view_weights is None:
        return
    call.dev_weights = []
    for i, entry in enumerate(call.view_weights):
        if entry is None:
            call.dev_weights.append(None)
            continue
        data, _, _ = _weight_tile(entry, call.views_bb[i], call.sdims, "fuse", i)
        dev = _resident_weight(data, call.device)
        if isinstance(entry, si_utils.SpatialImage) or msi_utils.is_msim(entry):
            sim = msi_utils.get_sim_from_msim(entry, scale="scale0") if msi_utils.is_msim(entry) else entry
            dev = si_utils.SpatialImage(dev, sim.dims, {d: np.asarray(sim.coords[d]) for d in sim.dims}, {"transforms": {}})
        call.dev_weights.append(dev)


class IndexFrameWarning(RuntimeWarning):
    """fuse_np was given a frame_origin it could not apply (an origin off the frame's grid)."""


# --- chunk -> view-slab plan (_core.py:354-722): computed by the library ---------------------------------
_PLAN_ENTRY = np.dtype([("block", "<i8", (3,)), ("view", "<i4"), ("planewise", "<i4"), ("lo", "<i8", (3,)), ("n", "<i8", (3,))])


def _plan_chunks(sparams, views_bb, output_stack_properties, output_chunksize, overlap_in_pixels, interpolation_order, sdims):
    """Which views, and which index window of each, feed which output chunk: one ``mvs_fuse_plan`` call (host code in the
    library, csrc/mvs_plan.hip) for the whole chunk grid.  Returns ``(by_block, info)``: ``by_block[block_index]`` =
    ``(planewise, [(iview, lo, n), ...])`` (views ascending; blocks without contributing views are absent) and ``info`` with
    the axes that are pure translations / lie on the views' sampling grid."""
    nd, nv = len(sdims), len(sparams)
    f64 = lambda rows: np.ascontiguousarray(rows, dtype=np.float64)
    i64 = lambda rows: np.ascontiguousarray(rows, dtype=np.int64)
    vo = f64([[vbb["origin"][d] for d in sdims] for vbb in views_bb]).reshape(nv, nd)
    vs = f64([[vbb["spacing"][d] for d in sdims] for vbb in views_bb]).reshape(nv, nd)
    vn = i64([[vbb["shape"][d] for d in sdims] for vbb in views_bb]).reshape(nv, nd)
    P = f64(np.stack([np.asarray(p, dtype=np.float64) for p in sparams])) if nv else np.zeros((0, nd + 1, nd + 1))
    try:
        Pinv = f64(np.linalg.inv(P)) if nv else P
    except np.linalg.LinAlgError:
        raise ValueError("a view's affine is singular") from None
    oo = f64([output_stack_properties["origin"][d] for d in sdims])
    osp = f64([output_stack_properties["spacing"][d] for d in sdims])
    on = i64([output_stack_properties["shape"][d] for d in sdims])
    cs = i64([output_chunksize[d] for d in sdims])
    halo = i64([overlap_in_pixels[d] for d in sdims])
    lib = _lib.load()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    count = C.c_int64(0)
    masks = (C.c_int32 * 2)()

    def call(buf, capacity):
        rc = lib.mvs_fuse_plan(nd, nv, dp(vo), dp(vs), ip(vn), dp(P), dp(Pinv), dp(oo), dp(osp), ip(on), ip(cs), ip(halo),
                               int(interpolation_order), buf, capacity, C.byref(count), masks)
        if rc != 0:
            raise RuntimeError(f"mvs_fuse_plan failed (code {rc})")

    call(None, 0)
    recs = np.zeros(max(int(count.value), 1), dtype=_PLAN_ENTRY)
    call(recs.ctypes.data_as(C.c_void_p), len(recs))
    recs = recs[: int(count.value)]
    by_block = {}
    blocks, views, pw = recs["block"][:, :nd].tolist(), recs["view"].tolist(), recs["planewise"].tolist()
    los, ns = recs["lo"][:, :nd].tolist(), recs["n"][:, :nd].tolist()
    for blk, v, p, lo, n in zip(blocks, views, pw, los, ns):
        by_block.setdefault(tuple(blk), (bool(p), []))[1].append((v, tuple(lo), tuple(n)))
    info = {"axis_aligned_translation_dims": [d for k, d in enumerate(sdims) if (masks[0] >> k) & 1],
            "grid_aligned_translation_dims": [d for k, d in enumerate(sdims) if (masks[1] >> k) & 1]}
    return by_block, info


_REPLAY = [True]           # tests / A-B: derive everything on every call
_HOST_STREAM = [os.environ.get("MVS_HOST_STREAM", "1") != "0"]            # fuse() of plain host arrays (>= 256 MiB) through the block pipeline
_HOST_STREAM_MIN_BYTES = 256 << 20
_STREAM_TILES = [os.environ.get("MVS_STREAM_TILES", "1") != "0"]            # fused blocks re-tiled on the device into chunk-major order before the download
_STREAM_PIPELINE = [os.environ.get("MVS_STREAM_PIPELINE", "1") != "0"]      # streaming.BlockPipeline around the launch blocks of a streamed fuse()
_REPLAY_MEMO = {}
_REPLAY_CAP = 32                     # geometries kept (8 ranks x a few mosaics; an entry is a few KB of view records)
_REPLAY_LOCK = threading.Lock()      # fuse() is also driven from one thread per GPU: lookups, evictions and inserts are serialised


def _hashable(v):
    if v is None or isinstance(v, (int, float, str, bool)):
        return v
    if isinstance(v, dict):
        return tuple(sorted((k, _hashable(x)) for k, x in v.items()))
    if isinstance(v, (list, tuple)):
        return tuple(_hashable(x) for x in v)
    if isinstance(v, np.ndarray):
        return (v.shape, str(v.dtype), v.tobytes())
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    raise TypeError


def _replay_key(images, transform_key, fusion_func, device, *args):
    """Everything fuse()'s host work depends on for device-resident plain images, as a hashable -- or None when the call is not
    of that kind.  Per image: the spatial dims, first / second coordinate and length of every axis (origin, spacing, shape as
    the stack-property getters read them), the transform under ``transform_key``, dtype, strides and device of the tile."""
    try:
        first = images[0]
        if msi_utils.is_msim(first) or fusion_func not in _FUSION_CODES:
            return None
        dims = tuple(first.dims)
        if any(d not in ("z", "y", "x") for d in dims):
            return None
        dtype = np.dtype(first.dtype)
        geo = np.empty((len(images), len(dims), 3))
        meta, trs = [], []
        for i, im in enumerate(images):
            data = im.data
            if msi_utils.is_msim(im) or tuple(im.dims) != dims or np.dtype(data.dtype) != dtype:
                return None
            if type(data).__name__ == "RemoteArray":
                # a tile this rank does not hold (sharding.RemoteArray: shape and dtype only): it takes part in the geometry; a
                # record is only made -- and replayed -- when none of the contributing views is one of these
                meta.append(("remote", tuple(data.shape)))
            elif is_device_array(data) and (data.device & 0xff) == (int(device) & 0xff):
                meta.append((data.shape, data.strides, data.device))
            else:
                return None
            co = im.coords
            for k, d in enumerate(dims):
                c = co[d]
                n = len(c)
                geo[i, k, 0], geo[i, k, 1], geo[i, k, 2] = c[0], (c[1] if n > 1 else c[0]), n
            trs.append(np.asarray(im.attrs["transforms"][transform_key], dtype=np.float64))
        shape0 = trs[0].shape
        if any(t.shape != shape0 for t in trs):
            return None
        return (dims, str(dtype), geo.tobytes(), np.stack(trs).tobytes(), shape0, tuple(meta), transform_key, fusion_func, int(device),
                tuple(_hashable(a) for a in args))
    except (KeyError, TypeError, AttributeError, IndexError):
        return None


def _replay_fuse(rec, images, transform_key, device):
    """fuse() from a remembered derivation: the view records with the CURRENT tiles' pointers, one mvs_fuse_chunk launch."""
    n = rec["n"]
    views = (_lib.mvs_view_t * n).from_buffer_copy(rec["views"])
    opts = _lib.mvs_fuse_opts_t.from_buffer_copy(rec["opts"])
    for iv in rec["view_index"]:
        images[iv].data.wait_ready(device)
    ptrs = np.array([images[iv].data.ptr for iv in rec["view_index"]], dtype=np.uint64) + rec["byte_offsets"]
    flat = np.frombuffer(views, dtype=np.uint8).reshape(n, C.sizeof(_lib.mvs_view_t))
    off = _lib.mvs_view_t.data.offset
    flat[:, off:off + 8].view(np.uint64)[:, 0] = ptrs
    out = DeviceArray.empty(rec["res_shape"], rec["dtype"], device)
    lib = _lib.init(device)
    rc = lib.mvs_fuse_chunk(device, views, n, C.byref(opts), C.c_void_p(out.ptr))
    _lib.check(rc, device, "mvs_fuse_chunk")
    out.mark_written()
    res = si_utils.to_spatial_image(out, dims=list(rec["dims"]), scale=rec["spacing"], translation=rec["origin"])
    si_utils.set_sim_affine(res, param_utils.identity_transform(rec["ndim"]), transform_key)
    return res


def _halo_overlap(overlap_in_pixels, sdims, funcs, output_chunksize):
    """The halo of fuse() (_core.py:1194-1222): the requested overlap per dim, raised to every function's
    ``required_overlap``; functions that accept ``output_chunksize`` get the requested chunk size among their kwargs."""
    overlap_in_pixels = overlap_in_pixels or 0
    if not isinstance(overlap_in_pixels, dict):
        overlap_in_pixels = {d: overlap_in_pixels for d in sdims}
    for func, kw in funcs:
        if func is not None and hasattr(func, "required_overlap"):
            kw = dict(kw or {})
            if has_keyword(func, "output_chunksize") and output_chunksize is not None:
                kw.setdefault("output_chunksize", output_chunksize)
            cur = func.required_overlap(kw)
            if not isinstance(cur, dict):
                cur = {d: cur for d in sdims}
            overlap_in_pixels = {d: max(overlap_in_pixels[d], cur[d]) for d in sdims}
    return overlap_in_pixels


class _FuseCall:
    """The state of one ``_fuse_once`` call; every step below reads and fills it.  The arguments of ``fuse()`` under their own
    names (``images`` with the ``sims`` alias resolved; ``batch_options`` / ``zarr_options`` as dicts once parsed), and:

    replay_key, record   key of the geometry-keyed replay, and the dict fuse_np records its launch in (None: not eligible)
    dev_weights          per view its ``view_weights`` tile resident on the device, or None (None altogether without the keyword)
    views                ``list(images)``, plain SpatialImages
    dtype                dtype of the views and of the result
    sdims, nsdims        spatial / non-spatial dims of the views
    ns_shape, n_fields   sizes of the non-spatial dims = the grid of (c, t) fields, and their number
    osp                  the output stack (origin, spacing, shape) as dict-of-dicts
    params, views_bb     per view: the affine under ``transform_key`` (may be t-stacked), the stack properties
    halo                 overlap per spatial dim a block is fused with (``_halo_overlap``)
    chunksize            the requested chunk size per spatial dim: the chunk grid of a Zarr output
    streamed             blocks pass through host memory one by one (Zarr in or out, large host arrays)
    block_size           size of a launch block: ``chunksize``, or whole multiples of it (``merge_chunks``)
    norm_chunks          per spatial axis the extents of the blocks in the result (with the halo when it is not trimmed)
    result_shape         spatial shape of the result: the output stack's, or the assembly of the untrimmed blocks
    blocks               per launch block ``block_index`` (its grid index), ``bb_halo`` (its box with the halo: what fuse_np
                         fuses) and ``window`` (the slices of the result it covers)
    zarr_out             the open output array (None without ``output_zarr_url``)
    ome_zarr             the output is level 0 of an NGFF image of version ``ngff_version``: the epilogue adds the pyramid
    result, dev_full     the host / the device result for all fields (None: the result is elsewhere)
    plans                per time point ``(affines, entries)``, see ``_plan_for``
    """

    def __init__(self, **arguments):
        self.__dict__.update(arguments)
        self.replay_key = self.record = self.zarr_out = self.result = self.dev_full = self.dev_weights = None
        self.ome_zarr, self.plans = False, {}


def _fuse_once(
    images=None,
    transform_key=None,
    fusion_func=weighted_average_fusion,
    fusion_func_kwargs=None,
    weights_func=None,
    weights_func_kwargs=None,
    output_spacing=None,
    output_stack_mode="union",
    output_origin=None,
    output_shape=None,
    output_stack_properties=None,
    output_chunksize=None,
    overlap_in_pixels=None,
    trim_overlap=True,
    interpolation_order=1,
    blending_widths=None,
    output_zarr_url=None,
    zarr_options=None,
    batch_options=None,
    backend="hip",
    output_on_backend=False,
    sims=None,
    device=0,
    chunk_filter=None,
    merge_chunks=True,
    frame_origin=None,
    view_weights=None,
):
    """Fuse input views (fusion.fuse, _core.py:782-1501), eagerly, on the HIP backend.

    Same arguments as the reference.  Differences forced by the environment:
    evaluation is eager (there is no dask) and ``images`` are numpy-,
    DeviceArray- or zarr-backed SpatialImages (``ngff_utils.read_sim_from_ome_zarr``;
    only the slab a chunk needs is read).  With ``output_zarr_url`` every
    fused chunk is written into a Zarr v2 array (``zarr_options``: ``ome_zarr``,
    ``ngff_version`` "0.4", ``overwrite``, ``zarr_array_creation_kwargs``) and
    the returned image is backed by that array.  Output chunks are fused one ``mvs_fuse_chunk`` call each,
    following the reference's chunk grid, halo and slab windows; the result is
    a SpatialImage with identity affine under ``transform_key``.
    ``chunk_filter(block_index) -> bool`` restricts the work to a subset of
    chunks (used by the multi-GPU farm); untouched chunks stay zero.
    ``merge_chunks``: with the built-in fusion functions and no halo the chunk grid is only the reference's unit of dask
    scheduling (and the chunk grid of a Zarr output) -- every output voxel is the same function of the views whichever
    chunk it falls in -- so the requested chunks are merged into launch blocks of whole chunks: up to ``MAX_LAUNCH_BYTES``
    of output for in-memory results (the whole mosaic when it fits: one ``mvs_fuse_chunk`` launch instead of hundreds), up to
    ``MAX_STREAM_BYTES`` when tiles are read from or the result is written to a Zarr store (a block is fused in one launch
    and written into its chunk files).  ``batch_options`` and ``chunk_filter`` address single chunks and switch this off.
    ``frame_origin``: origin of the index frame all chunks are fused in (see ``fuse_np``); default: the output stack's
    origin, so chunked, merged and unchunked runs of one stack agree voxel for voxel.  ``sharding.fuse_shard`` passes the
    origin of the WHOLE mosaic, so that every rank's sub-box equals the corresponding part of the single-GPU result.
    ``view_weights``: one feathered uint8 weight tile per view (``masks.feather`` of a mask; None for a view without one), see
    ``fuse_np``: "do not use this part of this view".  Every tile is uploaded once per call and every block gets the whole tiles
    of its views.  With the built-in fusion functions only; a ``weights_func``, ``multi_view_deconvolution``,
    ``multi_band_fusion``, user callables, multiscale images, weight tiles with ``t`` / ``c`` dims and plane-wise blocks are
    refused by name.  Such calls are left out of the geometry-keyed replay and of the block pipeline of streamed calls (their
    blocks are fused one after the other); ``fuse_to_host`` carries the keyword.
    """
    if images is None:
        if sims is None:
            raise TypeError("fuse() missing 1 required positional argument: 'images'")
        images = sims
    elif sims is not None:
        raise TypeError("fuse() got both 'images' and deprecated 'sims'. Use only 'images'.")
    if not images:
        raise ValueError("images must contain at least one image.")
    call = _FuseCall(
        images=images, transform_key=transform_key, fusion_func=fusion_func, fusion_func_kwargs=fusion_func_kwargs, weights_func=weights_func,
        weights_func_kwargs=weights_func_kwargs, output_spacing=output_spacing, output_stack_mode=output_stack_mode, output_origin=output_origin,
        output_shape=output_shape, output_stack_properties=output_stack_properties, output_chunksize=output_chunksize,
        overlap_in_pixels=overlap_in_pixels, trim_overlap=trim_overlap, interpolation_order=interpolation_order, blending_widths=blending_widths,
        output_zarr_url=output_zarr_url, zarr_options=zarr_options, batch_options=batch_options, backend=backend,
        output_on_backend=output_on_backend, device=device, chunk_filter=chunk_filter, merge_chunks=merge_chunks, frame_origin=frame_origin,
        view_weights=view_weights)
    if view_weights is not None:
        _check_view_weights_call(fusion_func, weights_func, "fuse")
        if len(view_weights) != len(images):
            raise ValueError(f"view_weights: one entry per view ({len(images)}), got {len(view_weights)}")
        if any(msi_utils.is_msim(im) for im in images):
            raise NotImplementedError("fuse: view_weights cannot be combined with multiscale images; fuse one scale with the tiles of that scale")
    hit = _replay_lookup(call)
    if hit is not None:
        return _replay_fuse(hit, images, transform_key, device)
    if output_zarr_url is not None and output_on_backend:
        raise ValueError("output_zarr_url streams chunks to disk; it cannot be combined with output_on_backend")
    if backend not in ("hip", None):
        raise ValueError("multiview_stitcher_amd.fusion.fuse only implements backend='hip'")
    is_ms = [msi_utils.is_msim(im) for im in images]
    if any(is_ms) and not all(is_ms):
        raise ValueError("All input images must be of the same kind: either all SpatialImages or all MultiscaleSpatialImages.")
    if all(is_ms):
        return _fuse_multiscale(call)
    _output_geometry(call)
    _launch_blocks(call)
    _chunk_grid(call)
    _check_batch_options(call)
    _open_zarr_output(call)
    _allocate_result(call)
    _upload_view_weights(call)
    if call.batch_options:
        _fuse_batches(call)
    else:
        for ns_index in np.ndindex(*call.ns_shape) if call.ns_shape else [()]:
            _fuse_field(call, ns_index)
    _record_replay(call)
    return _wrap_result(call)


def _replay_lookup(call):
    """Device-resident tiles fused into one device-resident launch block: everything the interpreter derives for the call --
    output stack, chunk plan, slab windows, the view records of mvs_fuse_chunk -- is a function of the views' geometry and the
    arguments, not of the voxels.  It is derived once per geometry and replayed with the current data pointers afterwards
    (a register + fuse loop over time points or channels of one mosaic pays the ~2 ms of host work once).  Returns the
    remembered derivation, or None after setting ``replay_key`` / ``record`` when this call may make one."""
    if not (_REPLAY[0] and call.output_on_backend and call.output_zarr_url is None and not call.batch_options and call.chunk_filter is None
            and call.merge_chunks and call.weights_func is None and not call.fusion_func_kwargs and not call.weights_func_kwargs
            and not call.zarr_options and call.backend in ("hip", None) and call.view_weights is None):
        return None
    call.replay_key = _replay_key(
        call.images, call.transform_key, call.fusion_func, call.device, call.output_spacing, call.output_stack_mode, call.output_origin,
        call.output_shape, call.output_stack_properties, call.output_chunksize, call.overlap_in_pixels, call.trim_overlap,
        call.interpolation_order, call.blending_widths, call.frame_origin)
    if call.replay_key is None:
        return None
    with _REPLAY_LOCK:
        hit = _REPLAY_MEMO.get(call.replay_key)
    if hit is None:
        call.record = {}
    return hit


def _fuse_multiscale(call):
    """MultiscaleSpatialImages in, a multiscale result out (fusion/_core.py:939-1064): scale0 defines the finest output
    geometry; every output level is FUSED (one ``fuse`` call) from the coarsest input level that is still fine enough for it
    (not downsampled from the level above); a Zarr output is one level fused from the matching input level."""
    common = {k: getattr(call, k) for k in (
        "transform_key", "fusion_func", "fusion_func_kwargs", "weights_func", "weights_func_kwargs", "output_stack_mode", "output_chunksize",
        "overlap_in_pixels", "trim_overlap", "interpolation_order", "blending_widths", "backend", "device", "chunk_filter", "merge_chunks")}
    scale0 = [msi_utils.get_sim_from_msim(m, scale="scale0") for m in call.images]
    sdims0 = si_utils.get_spatial_dims_from_sim(scale0[0])
    osp0 = _bb_dicts(process_output_stack_properties(scale0, call.output_spacing, call.output_origin, call.output_shape,
                                                     call.output_stack_properties, call.output_stack_mode, call.transform_key), sdims0)

    def level_sims(spacing):
        return [msi_utils.get_sim_from_msim(m, scale="scale%d" % msi_utils.get_res_level_from_spacing(m, spacing)) for m in call.images]

    if call.output_zarr_url is not None:
        fused = fuse(images=level_sims(osp0["spacing"]), output_stack_properties=osp0, output_zarr_url=call.output_zarr_url,
                     zarr_options=call.zarr_options, batch_options=call.batch_options, frame_origin=call.frame_origin, **common)
        if (call.zarr_options or {}).get("ome_zarr", False) and call.chunk_filter is None:
            return ngff_utils.read_msim_from_ome_zarr(
                call.output_zarr_url, transform_key=call.transform_key if call.transform_key is not None else si_utils.DEFAULT_TRANSFORM_KEY)
        return msi_utils.get_msim_from_sim(fused, scale_factors=[])
    shapes, _, abs_factors = msi_utils.calc_resolution_levels({d: int(osp0["shape"][d]) for d in sdims0})
    fused_levels = []
    for shape, f in zip(shapes, abs_factors):
        props = {"shape": dict(shape), "spacing": {d: osp0["spacing"][d] * f[d] for d in sdims0},
                 # centre-of-pixel convention of downsampled levels (as in the OME-Zarr pyramid)
                 "origin": {d: osp0["origin"][d] + (f[d] - 1) * osp0["spacing"][d] / 2 for d in sdims0}}
        # (a caller's frame_origin refers to the scale0 grid: a coarser level's grid is displaced by (f - 1) * spacing / 2
        # against it, so the level keeps its own frame = its own stack origin)
        level0 = all(int(f[d]) == 1 for d in sdims0)
        fused_levels.append(fuse(images=level_sims(props["spacing"]), output_stack_properties=props,
                                 output_on_backend=call.output_on_backend, frame_origin=call.frame_origin if level0 else None, **common))
    return msi_utils.get_msim_from_sims(fused_levels)


def _output_geometry(call):
    """The output stack, the dims, per view the affine and the box, the halo."""
    call.views = list(call.images)
    check_interpolation_order(call.interpolation_order, "interpolation_order")
    call.chunksize = process_output_chunksize(call.views, call.output_chunksize)
    osp = process_output_stack_properties(call.views, call.output_spacing, call.output_origin, call.output_shape,
                                          call.output_stack_properties, call.output_stack_mode, call.transform_key)
    call.sdims = si_utils.get_spatial_dims_from_sim(call.views[0])
    call.nsdims = si_utils.get_nonspatial_dims_from_sim(call.views[0])
    call.osp = _bb_dicts(osp, call.sdims)
    call.osp["shape"] = {d: int(v) for d, v in call.osp["shape"].items()}
    call.params = [si_utils.get_affine_from_sim(sim, call.transform_key) for sim in call.views]
    call.halo = _halo_overlap(call.overlap_in_pixels, call.sdims,
                              [(call.weights_func, call.weights_func_kwargs), (call.fusion_func, call.fusion_func_kwargs)], call.chunksize)
    call.views_bb = [si_utils.get_stack_properties_from_sim(sim) for sim in call.views]
    call.ns_shape = tuple(call.views[0].sizes[d] for d in call.nsdims)
    call.dtype = np.dtype(call.views[0].dtype)


def _launch_blocks(call):
    """Whether the call is streamed, and the size of its launch blocks."""
    kernel_fused = _kernel_fused(call.fusion_func, call.weights_func)
    single_blocks = bool(call.batch_options) or call.chunk_filter is not None      # (both address single chunks)
    call.streamed = call.output_zarr_url is not None or any(type(s.data).__name__ in ("ZarrArray", "ZarrView") for s in call.views)
    if not call.streamed and _HOST_STREAM[0] and _STREAM_PIPELINE[0] and not call.output_on_backend and not single_blocks and kernel_fused \
            and all(isinstance(s.data, np.ndarray) or is_device_array(s.data) for s in call.views) \
            and sum(int(np.prod(s.data.shape)) * np.dtype(s.dtype).itemsize for s in call.views) >= _HOST_STREAM_MIN_BYTES \
            and call.view_weights is None and _lib.device_count() > 0:
        # plain host arrays (or resident tiles) in, host array out -- what a user of the reference calls: launch blocks of <= 1 GiB through the block
        # pipeline (slabs copied into pinned staging buffers by the I/O pool, asynchronous transfers under the launch blocks, results
        # copied out by the pool) instead of ONE launch block whose views mvs_fuse_chunk uploads from pageable memory, fuses and
        # downloads one after the other: the north star 0.98 -> 0.41 s (2.26 -> 1.03 s for the first call of a process); resident tiles
        # with a host result 0.64 -> 0.24 s
        call.streamed = True
    call.block_size = call.chunksize
    if (call.merge_chunks and not single_blocks and kernel_fused and call.weights_func is None and not any(call.halo[d] for d in call.sdims)
            and not ("z" in call.sdims and int(call.chunksize["z"]) == 1 and call.osp["shape"]["z"] > 1)):
        # streamed inputs / outputs pass through host memory block by block: a smaller budget per launch block
        budget = _launch_budget(call.views, call.osp["shape"], call.sdims, call.dtype.itemsize, call.device,
                                MAX_STREAM_BYTES if call.streamed else MAX_LAUNCH_BYTES,
                                **({} if call.view_weights is None else {"view_weights": call.view_weights}))
        call.block_size = _merged_chunksize(call.chunksize, call.osp["shape"], call.sdims, call.dtype.itemsize, budget)


def _chunk_grid(call):
    """The launch blocks (``blocks``), and the shape of the result they tile."""
    sdims, halo, osp = call.sdims, call.halo, call.osp
    chunk_bbs, block_indices = mv_graph.get_chunk_bbs(osp, call.block_size)
    call.norm_chunks = mv_graph.normalize_chunks([call.block_size[d] for d in sdims], [osp["shape"][d] for d in sdims])
    call.result_shape = tuple(osp["shape"][d] for d in sdims)
    if (not call.trim_overlap) and any(halo[d] for d in sdims):
        # trim_overlap=False (_core.py:1252-1254, 1687-1711): every chunk keeps its halo and the result is the block
        # assembly of the untrimmed chunks side by side (da.block of chunks of shape chunk + 2 * halo), i.e. an array
        # that is larger than the output stack by 2 * halo per chunk and axis
        if call.output_zarr_url is not None:
            raise NotImplementedError("trim_overlap=False assembles untrimmed chunks in memory; it cannot stream to a Zarr store")
        call.norm_chunks = [tuple(int(n) + 2 * int(halo[d]) for n in cs_) for cs_, d in zip(call.norm_chunks, sdims)]
        call.result_shape = tuple(int(sum(n)) for n in call.norm_chunks)
    offsets = [np.cumsum((0,) + n[:-1]) for n in call.norm_chunks]
    call.blocks = [
        {"block_index": tuple(bi),
         "bb_halo": cb | {"origin": {d: cb["origin"][d] - halo[d] * osp["spacing"][d] for d in sdims}}
                       | {"shape": {d: cb["shape"][d] + 2 * halo[d] for d in sdims}},
         "window": tuple(slice(int(offsets[i][b]), int(offsets[i][b]) + int(call.norm_chunks[i][b])) for i, b in enumerate(bi))}
        for cb, bi in zip(chunk_bbs, block_indices)]


def _check_batch_options(call):
    """batch_options (_core.py:1068-1141, 2044-2156): with a Zarr output the reference hands batches of block ids to
    batch_func(fuse_chunk, block_ids, **batch_func_kwargs); fuse_chunk(block_id) fuses one block and writes its region."""
    call.batch_options = dict(call.batch_options or {})
    unknown = set(call.batch_options) - {"batch_func", "n_batch", "batch_func_kwargs"}
    if unknown:
        raise TypeError(f"unknown batch_options keys {sorted(unknown)}")
    if call.batch_options and call.output_zarr_url is None:
        raise ValueError("batch_options drive the block-wise Zarr output of fuse(); pass output_zarr_url as well")
    if call.batch_options and call.chunk_filter is not None:
        raise ValueError("batch_options and chunk_filter both select blocks; use one of them")


def _open_zarr_output(call):
    """Streaming output (_core.py:1068-1171, 2044-2156): every fused block goes straight into its region of a Zarr array
    (``zarr_out``), the mosaic never exists in host memory; with ome_zarr=True the array is level "0" of an NGFF image.  All
    checks come before the store is touched."""
    if call.output_zarr_url is None:
        return
    sdims, nsdims = call.sdims, call.nsdims
    call.zarr_options = dict(call.zarr_options or {})
    call.ome_zarr = bool(call.zarr_options.get("ome_zarr", False))
    call.ngff_version = call.zarr_options.get("ngff_version", "0.4")
    create_kw = dict(call.zarr_options.get("zarr_array_creation_kwargs") or {})
    store_chunksize = call.chunksize          # the chunk grid of a Zarr output stays the requested one
    if create_kw.get("chunks") is not None:
        # the store's chunk grid: full rank (c, t, spatial) or spatial dims only, as write_sim_to_ome_zarr takes it.  Every
        # fused block is written into its region, so the fuse chunk grid must be made of whole store chunks.
        req = [int(v) for v in create_kw["chunks"]]
        if len(req) == len(nsdims) + len(sdims):
            req = req[len(nsdims):]
        if len(req) != len(sdims) or min(req) < 1:
            raise ValueError(f"zarr_array_creation_kwargs['chunks'] {create_kw['chunks']} does not match dims {list(nsdims) + list(sdims)}")
        for d, n in zip(sdims, req):
            if int(call.chunksize[d]) % n and int(call.chunksize[d]) < int(call.osp["shape"][d]):
                raise ValueError(f"store chunks {req} do not tile the fuse chunks {[int(call.chunksize[d_]) for d_ in sdims]}")
        store_chunksize = dict(zip(sdims, req))
    create_kw.pop("chunks", None)
    if call.ome_zarr:
        want_fmt = 3 if str(call.ngff_version) == "0.5" else 2
        if int(create_kw.get("zarr_format", want_fmt)) != want_fmt:
            raise ValueError(f"zarr_format {create_kw['zarr_format']} conflicts with NGFF {call.ngff_version} "
                             f"(which stores Zarr v{want_fmt} arrays)")
    if call.zarr_options.get("overwrite", True) and os.path.exists(call.output_zarr_url) and call.chunk_filter is None:
        shutil.rmtree(call.output_zarr_url)
    if call.ome_zarr:
        create_kw = ngff_utils.update_zarr_array_creation_kwargs_for_ngff_version(call.ngff_version, create_kw)
        zarr_io.create_group(call.output_zarr_url, **ngff_utils.zarr_group_creation_kwargs_for_ngff_version(call.ngff_version))
        if create_kw.get("zarr_format") == 3:
            create_kw.setdefault("dimension_names", list(nsdims) + list(sdims))
    store_url = os.path.join(call.output_zarr_url, "0") if call.ome_zarr else call.output_zarr_url
    if zarr_io.array_exists(store_url):
        call.zarr_out = zarr_io.ZarrArray.open(store_url)      # a farm worker joining an array another worker created
    else:
        call.zarr_out = zarr_io.ZarrArray.create(
            store_url, call.ns_shape + call.result_shape, (1,) * len(call.ns_shape) + tuple(store_chunksize[d] for d in sdims), call.dtype,
            **create_kw)


def _allocate_result(call):
    """The host result, or with output_on_backend one device array for all (c, t) fields (_core.py:1275-1306 loops the
    fields): every field is fused into its own contiguous sub-array; a single field keeps the spatial dims only."""
    call.n_fields = int(np.prod(call.ns_shape)) if call.ns_shape else 1
    if call.output_on_backend:
        call.dev_full = DeviceArray.empty((call.ns_shape if call.n_fields > 1 else ()) + call.result_shape, call.dtype, call.device)
    elif call.zarr_out is None:
        call.result = np.zeros(call.ns_shape + call.result_shape, dtype=call.dtype)


def _plan_for(call, it):
    """(affines of time point ``it``, entries): by grid index and in block order, every launch block with the contributing
    views and the index window of each (``views``: [(iview, lo, n)], from ``mvs_fuse_plan``) and ``fuse_planewise``."""
    key = it if any(np.asarray(p).ndim == 3 for p in call.params) else 0
    if key not in call.plans:
        sparams = [param_utils.select_time(p, it) for p in call.params]
        by_block, _ = _plan_chunks(sparams, call.views_bb, call.osp, call.block_size, call.halo, call.interpolation_order, call.sdims)
        entries = {}
        for block in call.blocks:
            planewise, views = by_block.get(block["block_index"], (False, []))
            entries[block["block_index"]] = dict(block, views=views, fuse_planewise=planewise)
        call.plans[key] = (sparams, entries)
    return call.plans[key]


def _chunk_call(call, ns_index, entry, device):
    """fuse_np arguments of one (field, block)."""
    ns_sel = {d: int(i) for d, i in zip(call.nsdims, ns_index)}
    sparams, _ = _plan_for(call, ns_sel.get("t", 0))
    slabs = [call.views[iv].isel(dict(ns_sel, **{d: slice(a, a + m) for d, a, m in zip(call.sdims, lo, n)})) for iv, lo, n in entry["views"]]
    idxs = [iv for iv, _, _ in entry["views"]]
    params, cbb, fvb = [sparams[iv] for iv in idxs], entry["bb_halo"], [call.views_bb[iv] for iv in idxs]
    if entry["fuse_planewise"]:      # (one z plane on the views' z grid: a 2D chunk)
        slabs, params = [s.isel({"z": 0}) for s in slabs], [p[1:, 1:] for p in params]
        cbb, fvb = mv_graph.project_bb_along_dim(cbb, "z"), [mv_graph.project_bb_along_dim(b, "z") for b in fvb]
    kwargs = dict(
        sims=slabs, params=params, output_properties=cbb, fusion_func=call.fusion_func, fusion_func_kwargs=call.fusion_func_kwargs,
        weights_func=call.weights_func, weights_func_kwargs=call.weights_func_kwargs,
        trim_overlap_in_pixels=(call.halo if call.trim_overlap else 0), interpolation_order=call.interpolation_order, full_view_bbs=fvb,
        blending_widths=call.blending_widths, shrink_distance=0, backend="hip", device=device, _cb_check=False)
    kernel_fused = _kernel_fused(call.fusion_func, call.weights_func)
    if kernel_fused or call.fusion_func is multi_band_fusion:      # (the multi-band pyramids decimate on the frame's lattice)
        origin = call.frame_origin if call.frame_origin is not None else call.osp["origin"]
        kwargs["frame_origin"] = {d: origin[d] for d in cbb["origin"]}
        if kernel_fused and call.record is not None and not entry["fuse_planewise"]:
            kwargs["_record"] = call.record
            call.record["calls"] = call.record.get("calls", 0) + 1
            call.record["view_index"] = idxs
    if call.dev_weights is not None:
        if entry["fuse_planewise"]:
            raise NotImplementedError("fuse: view_weights cannot be combined with plane-wise blocks (an output chunk of one z plane on the "
                                      "views' z grid is fused as a 2D chunk); choose an output_chunksize of more than one plane")
        kwargs["view_weights"] = [call.dev_weights[iv] for iv in idxs]
    return kwargs


def _deliver(call, ns_index, entry, chunk, pipelined=False):
    """A fused host block into its region of the Zarr output or its window of the host result (``pipelined``: called by the
    block pipeline's writer, which copies and writes through the I/O pool).  A plane-wise block gets its plane axis back."""
    if entry["fuse_planewise"]:
        chunk = chunk[np.newaxis]
    if call.zarr_out is not None:
        start, data = list(ns_index) + [s.start for s in entry["window"]], chunk.reshape((1,) * len(ns_index) + chunk.shape)
        if pipelined:
            streaming.write_region(call.zarr_out, start, data)
        else:
            call.zarr_out.write(start, data)
    elif pipelined:
        streaming.parallel_copy(call.result[tuple(ns_index) + entry["window"]], chunk, kind="write")
    elif chunk.shape == call.result.shape:
        call.result = chunk           # one launch block and one field: the fused array is the result
    else:
        call.result[tuple(ns_index) + entry["window"]] = chunk


def _fuse_batches(call):
    """Block-wise Zarr output driven by ``batch_func``: batches of ``n_batch`` block ids in ``np.ndindex`` order."""
    def fuse_chunk(block_id, device=call.device):
        """Fuse block ``block_id`` (index into the chunk grid of the output array, non-spatial axes first) and write
        it into its region of the output store; ``device`` lets a batch function place blocks on several GPUs."""
        block_id, n_ns = tuple(int(b) for b in block_id), len(call.ns_shape)
        ns_index = block_id[:n_ns]
        entry = _plan_for(call, dict(zip(call.nsdims, ns_index)).get("t", 0))[1][block_id[n_ns:]]
        if entry["views"]:      # (the store's fill value (0) stands for blocks without contributing views)
            _deliver(call, ns_index, entry, np.asarray(fuse_np(**_chunk_call(call, ns_index, entry, device))))

    batch_func = call.batch_options.get("batch_func") or (lambda func, block_ids, **_: [func(b) for b in block_ids])
    n_batch = int(call.batch_options.get("n_batch", 1))
    block_iter = iter(np.ndindex(*(tuple(call.ns_shape) + tuple(len(n) for n in call.norm_chunks))))
    while True:
        batch = [b for _, b in zip(range(n_batch), block_iter)]
        if not batch:
            break
        batch_func(fuse_chunk, batch, **(call.batch_options.get("batch_func_kwargs") or {}))


def _fuse_field(call, ns_index):
    """All blocks of one (c, t) field.  A block is fused in one of three ways: submitted to the block pipeline, into the
    device result, or on the host."""
    entries = list(_plan_for(call, dict(zip(call.nsdims, (int(i) for i in ns_index))).get("t", 0))[1].values())

    def selected(entry):      # (blocks the filter rejects and blocks without contributing views are not fused)
        return (call.chunk_filter is None or call.chunk_filter(entry["block_index"])) and bool(entry["views"])

    if call.dev_full is not None:
        dev_out = call.dev_full[tuple(int(i) for i in ns_index)] if call.n_fields > 1 else call.dev_full
        # one block that is actually fused over the whole array writes every voxel; in every other case (several blocks,
        # a block without views, a block the filter rejects) untouched voxels must read 0 like the host result
        single = len(entries) == 1 and bool(entries[0]["views"]) and selected(entries[0])
        if not single:
            dev_out.fill_zero()
    # tiles read from Zarr stores and / or a result that leaves the device block by block: read-ahead, asynchronous transfers
    # and write-behind around the launch blocks (streaming.BlockPipeline) -- the same fuse_np calls in the same order
    pipelined = (call.streamed and _STREAM_PIPELINE[0] and call.dev_full is None and _kernel_fused(call.fusion_func, call.weights_func)
                 and call.view_weights is None and _lib.device_count() > 0)
    pipe = streaming.BlockPipeline(fuse_np, call.device) if pipelined else None
    try:
        for entry in entries:
            if not selected(entry):
                continue
            kwargs = _chunk_call(call, ns_index, entry, call.device)
            if pipe is not None:
                tiled = call.zarr_out is not None and not entry["fuse_planewise"] and _STREAM_TILES[0]
                tiling = (call.zarr_out, list(ns_index) + [s.start for s in entry["window"]]) if tiled else None
                pipe.submit(kwargs, functools.partial(_deliver, call, ns_index, entry, pipelined=True), tiling)
            elif call.dev_full is None:
                _deliver(call, ns_index, entry, np.asarray(fuse_np(**kwargs)))
            elif single:
                # (a plane-wise entry is fused with 2D parameters: hand it the one plane of the 3D result)
                fuse_np(out=dev_out[0] if entry["fuse_planewise"] else dev_out, **kwargs)
            else:
                # chunked workflow with a device-resident mosaic: every block is fused on the device and copied into
                # its window of the mosaic device-to-device (stream-ordered, no host round trip)
                fuse_np(output_on_backend=True, **kwargs).copy_into(dev_out, [s.start for s in entry["window"]])
    except BaseException:
        if pipe is not None:
            pipe.abort()      # (queued reads are dropped, the stage threads end; the error of the block that failed goes up)
        raise
    if pipe is not None:
        pipe.finish()


def _record_replay(call):
    """One launch block wrote the whole device result: remember its derivation under ``replay_key``.  Slab pointers are
    remembered as offsets into their tiles."""
    record = call.record
    if not (record is not None and record.get("calls") == 1 and "views" in record and not record.get("no_replay") and not call.nsdims
            and call.n_fields == 1 and tuple(call.dev_full.shape) == record["res_shape"]):
        return
    base = np.array([call.images[iv].data.ptr for iv in record["view_index"]], dtype=np.uint64)      # (all device-resident: fuse_np recorded)
    entry = dict(record, byte_offsets=(record["ptrs"] - base).astype(np.uint64), dims=tuple(call.sdims),
                 spacing=dict(call.osp["spacing"]), origin=dict(call.osp["origin"]), dtype=np.dtype(call.images[0].dtype), ndim=len(call.sdims))
    with _REPLAY_LOCK:
        while len(_REPLAY_MEMO) >= _REPLAY_CAP:
            _REPLAY_MEMO.pop(next(iter(_REPLAY_MEMO)), None)      # (oldest first: dicts keep insertion order)
        _REPLAY_MEMO[call.replay_key] = entry


def _wrap_result(call):
    """The result as a SpatialImage with identity affine under ``transform_key``; for an OME-Zarr output the pyramid levels
    and multiscales metadata around the level-0 array the blocks were written into (_core.py:1160-1171)."""
    dims = list(call.nsdims) + list(call.sdims)
    if call.dev_full is not None:
        call.dev_full.mark_written()
        data, dims = call.dev_full, (dims if call.n_fields > 1 else list(call.sdims))
    else:
        data = call.result if call.zarr_out is None else call.zarr_out[...]
    res = si_utils.to_spatial_image(
        data, dims=dims, scale=call.osp["spacing"], translation=call.osp["origin"],
        c_coords=call.views[0].coords.get("c") if "c" in dims else None,
        t_coords=call.views[0].coords.get("t") if "t" in dims else None,
    )
    si_utils.set_sim_affine(res, param_utils.identity_transform(len(call.sdims)), call.transform_key)
    if call.zarr_out is not None and call.ome_zarr and call.chunk_filter is None:
        res = ngff_utils.write_sim_to_ome_zarr(res, call.output_zarr_url, overwrite=False, ngff_version=call.ngff_version,
                                               zarr_array_creation_kwargs=call.zarr_options.get("zarr_array_creation_kwargs"),
                                               device=call.device)
    return res


def fuse(*args, **kwargs):
    bound = inspect.signature(_fuse_once).bind(*args, **kwargs)      # wherever merge_chunks was passed, it can be overridden
    try:
        res = _fuse_once(*bound.args, **bound.kwargs)
        if bound.arguments.get("weights_func") is content_based and bound.arguments.get("output_on_backend"):
            # chunks left on the device are not waited for one by one; a mask list of the fast content-based path that overflowed
            # in any of them shows here, and the mosaic is fused again through the bit-faithful passes
            dev_ = bound.arguments.get("device", 0)
            if _cb_overflowed(dev_):
                with _library_option("cb_exact", dev_):
                    res = _fuse_once(*bound.args, **bound.kwargs)
        return res
    except _lib.DeviceMemoryError as exc:
        # A merged launch block is sized from an ESTIMATE of what has to be staged on the device (_launch_budget); if the
        # device still runs out of memory the requested chunk grid -- the unit the caller sized for -- is used instead.
        if not bound.arguments.get("merge_chunks", True):
            raise
        failure = str(exc)
        # the retry must not run inside this handler: the traceback keeps the failed attempt's frames -- and with them the
        # mosaic-sized device buffer, staged peer copies and keep lists -- alive on a device that has just run out of memory
        traceback.clear_frames(exc.__traceback__)
    gc.collect()
    warnings.warn(f"fuse(): a merged launch block did not fit the device ({failure}); falling back to the requested "
                  "output_chunksize", RuntimeWarning, stacklevel=2)
    bound.arguments["merge_chunks"] = False
    return _fuse_once(*bound.args, **bound.kwargs)


fuse.__doc__ = _fuse_once.__doc__
fuse.__wrapped__ = _fuse_once


def fuse_to_host(images, transform_key=None, n_slabs=8, out=None, device=0, return_timeline=False, **fuse_kwargs):
    """``fuse()`` of views resident on (or on their way to) the device with the RESULT in host memory, the download overlapped with
    the kernels: the output stack is cut into ``n_slabs`` slabs along its first axis, every slab is fused in one launch block
    (``output_on_backend=True``) and copied into its window of a pinned host array on the device's copy stream while the next
    slab is fused (mvs_mark on the fuse lane -> mvs_copy_async, csrc/mvs_transfer.hip).  The reference streams fused chunks out of a
    dask graph into host memory / a Zarr store (_core.py:1068-1170, 2044-2156); SURVEY 8d(2)'s end-to-end figure includes this
    D2H.  Every slab is fused in the index frame of the WHOLE stack (``frame_origin``), so the result equals ``fuse()`` of the
    whole stack voxel for voxel.  ``out``: a pinned C-contiguous array of the result's shape (``device.pinned_empty``) to fill
    instead of a new one.  ``return_timeline``: also return [(fuse done, download done)] per slab in ms since the first slab's
    launch block was queued (timed tickets) -- the overlap test reads it.  Remaining keyword arguments: those of ``fuse()``
    (single field images: spatial dims only)."""
    for bad in ("output_zarr_url", "batch_options", "output_on_backend", "chunk_filter", "sims"):
        if fuse_kwargs.get(bad):
            raise TypeError(f"fuse_to_host does not take {bad}")
    images = list(images)
    sdims = si_utils.get_spatial_dims_from_sim(images[0])
    if list(images[0].dims) != list(sdims):
        raise ValueError("fuse_to_host fuses single fields (spatial dims only)")
    osp = _bb_dicts(process_output_stack_properties(
        images, fuse_kwargs.pop("output_spacing", None), fuse_kwargs.pop("output_origin", None), fuse_kwargs.pop("output_shape", None),
        fuse_kwargs.pop("output_stack_properties", None), fuse_kwargs.pop("output_stack_mode", "union"), transform_key), sdims)
    shape = tuple(int(osp["shape"][d]) for d in sdims)
    dtype = np.dtype(images[0].dtype)
    if out is None:
        out = dev_mod.pinned_empty(shape, dtype)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.flags.c_contiguous or not dev_mod.is_pinned(out):
        raise ValueError(f"out must be a pinned C-contiguous {dtype} array of shape {shape}")
    d0, n0 = sdims[0], shape[0]
    n_slabs = max(1, min(int(n_slabs), n0))
    cuts = np.linspace(0, n0, n_slabs + 1).round().astype(int)
    fuse_kwargs.setdefault("frame_origin", dict(osp["origin"]))
    fuse_kwargs.setdefault("output_chunksize", {d: 1 << 30 for d in sdims})
    t_start = dev_mod.mark(device)
    h_start = time.perf_counter()
    pending, timeline, host_ms = [], [], []      # host_ms: (fuse() of the slab entered, returned) on the host clock, ms
    # The class kernels of a slab's launch stay on the lane's own stream (option serial_classes) while downloads are in flight: forked
    # onto the LOW-priority side streams they were served only when the HIGH-priority copy stream's queue had drained -- slab k + 1 was
    # fused when slab k's download was through, in most runs for some slabs, in one run of ten for all of them, once 377 ms late
    # (A/B on one box, profiles/round6_summary.md 4).  A slab is 1/8 of a mosaic; forking saves it ~0.1 ms.  (The other half of the
    # same symptom: parameter blocks uploaded by a copy engine queued behind the downloads -- csrc/mvs_context.hip: mvs_upload_small.)
    with _library_option("serial_classes", device):
        for k in range(n_slabs):
            a, b = int(cuts[k]), int(cuts[k + 1])
            if b <= a:
                continue
            sub = {"origin": dict(osp["origin"], **{d0: osp["origin"][d0] + a * osp["spacing"][d0]}), "spacing": dict(osp["spacing"]),
                   "shape": dict(osp["shape"], **{d0: b - a})}
            h0 = time.perf_counter()
            fused = fuse(images, transform_key=transform_key, output_stack_properties=sub, output_on_backend=True, device=device, **fuse_kwargs)
            host_ms.append(((h0 - h_start) * 1e3, (time.perf_counter() - h_start) * 1e3))
            t_fused = dev_mod.mark(device)
            t_down = fused.data.download_async(out[a:b], after=t_fused)
            pending.append((fused, t_fused, t_down))      # (the slab stays alive until its download has passed)
        for fused, t_fused, t_down in pending:
            dev_mod.ticket_sync(t_down)
            if return_timeline:
                timeline.append((dev_mod.ticket_elapsed_ms(t_start, t_fused), dev_mod.ticket_elapsed_ms(t_start, t_down)))
        res = si_utils.to_spatial_image(out, dims=list(sdims), scale=osp["spacing"], translation=osp["origin"])
        si_utils.set_sim_affine(res, param_utils.identity_transform(len(sdims)), transform_key)
    fuse_to_host.last_host_ms = host_ms          # (measurement: where the host was while the slabs were queued)
    return (res, timeline) if return_timeline else res
