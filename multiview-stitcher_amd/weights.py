"""Blending / fusion weights on the HIP backend (mirror of the reference's weights.py).

Host side: the 5^ndim blending support (weights.py:430-470) and its pixel-space
affine; device side: resample + cosine ramp fused into ``mvs_fuse_chunk``
(csrc/mvs_fuse.hip), or as a standalone volume through ``mvs_blend_weights``.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._operands import dense_operand, embed3, result_array, shape3, written
from .transformation import _as_zyx, get_pixel_affine

DEFAULT_BLENDING_WIDTHS = {"z": 3, "y": 10, "x": 10}


def content_based_required_overlap(sigma_2=11, **_):
    """``@requires_overlap(lambda kwargs: 2 * kwargs["sigma_2"])`` of weights.py:22."""
    return 2 * sigma_2


def _shrink_source_bb(origin, spacing, shape, shrink_distance, sdims):
    """weights._shrink_source_bb (weights.py:348-388)."""
    if isinstance(shrink_distance, dict):
        sd = np.array([float(shrink_distance.get(d, 0)) for d in sdims])
    else:
        sd = np.full(len(sdims), float(shrink_distance))
    return origin + sd, spacing, shape - 2 * sd / spacing


_TABLE_CACHE = {}


def blending_support(source_bb, blending_widths=None, shrink_distance=0):
    """The EDT support image of get_blending_weights (weights.py:430-470).

    Returns (table float32 (5,)*ndim, support origin, support spacing as read
    back from the SpatialImage coordinates).  The table is the closed form of
    ``distance_transform_edt(mask, sampling)`` for the fixed 5^n mask whose inner
    3^n block is foreground: the nearest background voxel of an inner voxel lies
    straight along one axis, so  edt[i] = min_d( min(i_d, 4 - i_d) * sampling_d ).
    """
    sdims = sorted(source_bb["origin"].keys())[::-1] if isinstance(source_bb["origin"], dict) else ["z", "y", "x"][-len(source_bb["origin"]):]
    ndim = len(sdims)
    if blending_widths is None:
        blending_widths = DEFAULT_BLENDING_WIDTHS
    bw = _as_zyx(blending_widths, sdims)
    origin = _as_zyx(source_bb["origin"], sdims)
    spacing = _as_zyx(source_bb["spacing"], sdims)
    shape = _as_zyx(source_bb["shape"], sdims)
    if (isinstance(shrink_distance, dict) and any(shrink_distance.values())) or (
        not isinstance(shrink_distance, dict) and shrink_distance
    ):
        origin, spacing, shape = _shrink_source_bb(origin, spacing, shape, shrink_distance, sdims)
    support_spacing = (shape - 1) / 4 * spacing
    edt_support_spacing = support_spacing * (shape - 1 + 2 * 1) / (shape - 1)
    edt_support_origin = origin - 1 * spacing
    sampling = edt_support_spacing / bw
    key = tuple(sampling.tolist())
    table = _TABLE_CACHE.get(key)
    if table is None:      # all tiles of a mosaic share one table
        tent = np.minimum(np.arange(5), 4 - np.arange(5)).astype(np.float64)
        per_axis = [tent * sampling[d] for d in range(ndim)]
        grids = np.meshgrid(*per_axis, indexing="ij")
        table = np.minimum.reduce(grids).astype(np.float32)
        if len(_TABLE_CACHE) > 64:
            _TABLE_CACHE.clear()
        _TABLE_CACHE[key] = table
    # origin/spacing as the reference reads them back from the coordinate arrays
    # (spatial_image_utils.py:316-317, 554-589): coords = o + s*arange(5)
    c0 = edt_support_origin + edt_support_spacing * 0.0
    c1 = edt_support_origin + edt_support_spacing * 1.0
    return table, c0, c1 - c0


def blending_supports(origins, spacings, shapes, sdims, blending_widths=None, shrink_distance=0):
    """``blending_support`` for a stack of views ((n, ndim) arrays in ``sdims`` order): (tables, support origins, support
    spacings); views with the same sampling share one table object."""
    ndim = len(sdims)
    if blending_widths is None:
        blending_widths = DEFAULT_BLENDING_WIDTHS
    bw = _as_zyx(blending_widths, sdims)
    origin, spacing, shape = (np.asarray(a, dtype=np.float64) for a in (origins, spacings, shapes))
    if (isinstance(shrink_distance, dict) and any(shrink_distance.values())) or (
        not isinstance(shrink_distance, dict) and shrink_distance
    ):
        origin, spacing, shape = _shrink_source_bb(origin, spacing, shape, shrink_distance, sdims)
    support_spacing = (shape - 1) / 4 * spacing
    edt_support_spacing = support_spacing * (shape - 1 + 2 * 1) / (shape - 1)
    edt_support_origin = origin - 1 * spacing
    sampling = edt_support_spacing / bw
    tables = []
    for row in sampling:
        key = tuple(row.tolist())
        table = _TABLE_CACHE.get(key)
        if table is None:
            tent = np.minimum(np.arange(5), 4 - np.arange(5)).astype(np.float64)
            grids = np.meshgrid(*[tent * row[d] for d in range(ndim)], indexing="ij")
            table = np.minimum.reduce(grids).astype(np.float32)
            if len(_TABLE_CACHE) > 64:
                _TABLE_CACHE.clear()
            _TABLE_CACHE[key] = table
        tables.append(table)
    c0 = edt_support_origin + edt_support_spacing * 0.0
    c1 = edt_support_origin + edt_support_spacing * 1.0
    return tables, c0, c1 - c0


def fill_view_weights(view, source_bb, affine, target_origin, target_spacing, blending_widths=None, shrink_distance=0):
    """Fill the blending half of an ``mvs_view_t`` (w_matrix, w_offset, edt)."""
    table, sup_origin, sup_spacing = blending_support(source_bb, blending_widths, shrink_distance)
    ndim = table.ndim
    wm, wo = get_pixel_affine(np.linalg.inv(np.asarray(affine, dtype=np.float64)), sup_origin, sup_spacing,
                              target_origin, target_spacing)
    m3, o3 = embed3(wm, wo)
    view.w_matrix[:] = m3.reshape(-1).tolist()
    view.w_offset[:] = o3.tolist()
    flat = np.zeros(125, dtype=np.float32)
    flat[: table.size] = table.reshape(-1)
    C.memmove(view.edt, flat.ctypes.data, 500)
    return ndim


def get_blending_weights(target_bb, source_bb, affine, blending_widths=None, shrink_distance=0, device=0):
    """weights.get_blending_weights (weights.py:391-511): float32 volume on the target grid."""
    lib = _lib.init(device)
    sdims = sorted(source_bb["origin"].keys())[::-1] if isinstance(source_bb["origin"], dict) else ["z", "y", "x"][-len(source_bb["origin"]):]
    view = _lib.mvs_view_t()
    ndim = fill_view_weights(view, source_bb, affine, _as_zyx(target_bb["origin"], sdims),
                             _as_zyx(target_bb["spacing"], sdims), blending_widths, shrink_distance)
    out_shape = [int(v) for v in _as_zyx(target_bb["shape"], sdims)]
    out = np.empty(tuple(out_shape), dtype=np.float32)
    rc = lib.mvs_blend_weights(device, C.byref(view), ndim, _lib.i64x3(shape3(out_shape)), out.ctypes.data,
                               _lib.MVS_MEM_HOST)
    _lib.check(rc, device, "mvs_blend_weights")
    return out


def _clamp_overlap(overlap, output_chunksize):
    """weights._clamp_overlap (weights.py:514-524): the overlap per dim, at most the output chunk size."""
    sdims = sorted(output_chunksize.keys())[::-1]
    if not isinstance(overlap, dict):
        overlap = {dim: int(overlap) for dim in sdims}
    return {dim: min(overlap[dim], output_chunksize[dim]) for dim in sdims}


def content_based_dct_required_overlap(kwargs):
    """``@requires_overlap(lambda kwargs: _clamp_overlap(kwargs["dct_size"], kwargs["output_chunksize"]))`` of
    weights.py:70-84, with the defaults merged in as misc_utils.requires_overlap does."""
    kw = {"dct_size": 32, "output_chunksize": None, **(kwargs or {})}
    return _clamp_overlap(kw["dct_size"], kw["output_chunksize"])


def dct_opts(ndim, dct_size=32, exponent=1.0, otf_support_fraction=0.5, output_chunksize=None):
    """The ``mvs_dct_opts_t`` of content_based_dct's keyword arguments (spatial dims z, y, x; 2D: y, x)."""
    sdims = ["z", "y", "x"][-ndim:]
    o = _lib.mvs_dct_opts_t()
    sizes = [dct_size[d] for d in sdims] if isinstance(dct_size, dict) else [dct_size] * ndim
    for k, v in enumerate([1] * (3 - ndim) + [int(s) for s in sizes]):
        o.dct_size[k] = v
    if output_chunksize is not None:
        o.has_output_chunksize = 1
        for k, v in enumerate([1] * (3 - ndim) + [int(output_chunksize[d]) for d in sdims]):
            o.output_chunksize[k] = v
    o.exponent = float(exponent)
    if otf_support_fraction is not None:
        o.has_otf = 1
        o.otf_support_fraction = float(otf_support_fraction)
    return o


def content_based_dct(transformed_views, dct_size=32, exponent=1.0, otf_support_fraction=0.5, output_chunksize=None, device=0,
                      return_quality=False):
    """weights.content_based_dct (weights.py:77-290): DCT Shannon-entropy fusion weights on the device.

    ``transformed_views`` (n_views, *spatial) as numpy or ``DeviceArray`` (NaN = outside a view); returns float32 weights of
    the same shape and kind (``mvs_content_dct_weights``).  ``return_quality``: also the raw per-block qualities
    (n_views, *blocks), before the shift by their minimum over the views.
    """
    from .device import DeviceArray, is_device_array

    lib = _lib.init(device)
    on_dev = is_device_array(transformed_views)
    if on_dev and (transformed_views.dtype != np.float32 or not transformed_views.is_contiguous()):
        transformed_views = DeviceArray.from_host(np.ascontiguousarray(transformed_views.get(), dtype=np.float32), device)
    ptr, mem, views = dense_operand(transformed_views, (np.float32,), device, "content_based_dct", host_dtype=np.float32)
    nv, spatial = int(views.shape[0]), tuple(int(s) for s in views.shape[1:])
    ndim = len(spatial)
    if ndim not in (2, 3):
        raise ValueError("content_based_dct: transformed_views must be (n_views, y, x) or (n_views, z, y, x)")
    opts = dct_opts(ndim, dct_size, exponent, otf_support_fraction, output_chunksize)
    s3 = shape3(spatial)
    sizes = [opts.dct_size[k] for k in range(3)]
    if opts.has_output_chunksize:
        sizes = [min(sizes[k], opts.output_chunksize[k]) for k in range(3)]
    nblocks = tuple(max(1, -(-s3[k] // min(sizes[k], s3[k]))) for k in range(3 - ndim, 3))
    out, optr, _ = result_array((nv,) + spatial, np.float32, on_dev, device)
    q, qptr, _ = result_array((nv,) + nblocks, np.float32, on_dev, device) if return_quality else (None, None, None)
    rc = lib.mvs_content_dct_weights(device, C.c_void_p(ptr), nv, _lib.i64x3(s3), ndim, C.byref(opts), C.c_void_p(optr), C.c_void_p(qptr), mem)
    _lib.check(rc, device, "mvs_content_dct_weights")
    written(out)
    written(q)
    return (out, q) if return_quality else out


content_based_dct.required_overlap = content_based_dct_required_overlap
