"""Sample masks and mask-driven pair selection on the GPU.

On a sparse specimen most overlaps of a large mosaic are empty, and a phase correlation of an empty overlap reports a spurious
shift.  This module says where the sample is: one Otsu threshold for the whole acquisition (``otsu_threshold``), a binary mask per
tile (``sample_masks``), the fusion of the label images ``mask_i * (i + 1)`` by their minimum at interpolation order 0
(``fuse_labels``) and the list of the labels that touch (``contact_pairs``).  ``registration.get_pairs_from_sample_masks`` and
``mv_graph.get_connected_labels`` compose them under the reference's names (registration.py:3256-3292, mv_graph.py:895-931); the
pair list goes into ``registration.register(..., pairs=)``.  The same masks can keep parts of a view out of the mosaic: ``feather``
turns a mask into a feathered weight tile for ``fusion.fuse(..., view_weights=)``.

All voxel work runs in HIP kernels (csrc/mvs_masks.hip, csrc/mvs_mask_feather.hip; include/mvs_hip.h states their rules and limits); every result is an
integer or a selection, so equal inputs give equal bits.  2-D and 3-D; tiles in host memory or resident on the device; sims with
``t`` or ``c`` dims are refused (select a time point and a channel first).
"""

from __future__ import annotations

import numpy as np

from . import _detect_ops, _lib, _mask_ops, fusion, msi_utils, param_utils
from . import spatial_image_utils as si_utils
from .device import is_device_array
from .mv_graph import otsu_from_histogram  # noqa: F401  (public here: the arithmetic mv_graph.threshold_otsu shares)
from .transformation import get_pixel_affines


def _spatial_sim(image, who):
    """The full-resolution spatial image of a view; a ``t`` or ``c`` dim is refused by name."""
    sim = msi_utils.get_sim_from_msim(image, scale="scale0") if msi_utils.is_msim(image) else image
    for d in sim.dims:
        if d in ("t", "c"):
            raise ValueError(f"{who}: a sim with a {d!r} dim is not supported; select one index of {d!r} first")
    if len(si_utils.get_spatial_dims_from_sim(sim)) not in (2, 3):
        raise ValueError(f"{who}: sims are 2-D or 3-D")
    return sim


def _per_axis(value, sdims, name):
    """``value`` (None, one number, a dict that may leave dims out, or one number per dim) as a list over ``sdims``, or None."""
    if value is None:
        return None
    if isinstance(value, dict):
        return [value.get(d, 0) for d in sdims]
    if np.ndim(value) == 0:
        return [value] * len(sdims)
    if len(value) != len(sdims):
        raise ValueError(f"{name}: one value, or one per spatial dim ({len(sdims)})")
    return list(value)


def _condition(sim, binning, sigma, device):
    """A tile as it is thresholded: block means over ``binning`` (``registration._bin_sim``: the tile's dtype, the binned
    coordinates), then Gaussian smoothing with ``sigma`` pixels of the binned tile (mvs_log_response without second-order taps:
    float32 on the device)."""
    from . import registration

    sdims = si_utils.get_spatial_dims_from_sim(sim)
    if binning is not None:
        bins = _per_axis(binning, sdims, "binning")
        if any(int(b) < 1 for b in bins):
            raise ValueError("binning factors must be >= 1")
        sim = registration._bin_sim(sim, {d: max(int(b), 1) for d, b in zip(sdims, bins)}, device)
    sigmas = _per_axis(sigma, sdims, "sigma")
    if sigmas is not None and any(float(s) > 0 for s in sigmas):
        if any(float(s) <= 0 for s in sigmas):
            raise ValueError("sigma must be positive on every axis (or None)")
        data = sim.data
        if is_device_array(data) and not data.is_contiguous():
            raise TypeError("smoothing needs contiguous device tiles")
        sim = sim.copy(data=_detect_ops.gaussian_smooth(data, [float(s) for s in sigmas], device))
    return sim


def _spatial_sims(msims_or_sims, who):
    sims = [_spatial_sim(m, who) for m in msims_or_sims]
    if not sims:
        raise ValueError(f"{who}: no tiles")
    return sims


def _otsu_of_tiles(tiles, n_bins, device):
    lo, hi, n = _mask_ops.value_range(tiles, device)
    if n == 0:
        raise ValueError("otsu_threshold: the tiles hold no voxel that is not NaN")
    if lo == hi:
        return lo
    return float(otsu_from_histogram(_mask_ops.histogram(tiles, n_bins, lo, hi, device), lo, hi))


def otsu_threshold(msims_or_sims, n_bins=256, sigma=None, binning=None, device=0):
    """One Otsu threshold for all tiles of an acquisition: ``mv_graph.threshold_otsu`` of all their voxels together, NaNs left
    out.  Minimum and maximum come from one pass of mvs_tile_histogram, the exact ``n_bins`` counts of
    ``np.histogram(values, n_bins, (min, max))`` from a second one, the threshold from ``otsu_from_histogram`` on the host.
    ``binning`` / ``sigma``: the tiles are first conditioned as ``sample_masks`` conditions them.  ``n_bins <= 4096``."""
    n_bins = _mask_ops.check_n_bins(n_bins)
    tiles = [_condition(s, binning, sigma, device).data for s in _spatial_sims(msims_or_sims, "otsu_threshold")]
    return _otsu_of_tiles(tiles, n_bins, device)


def sample_masks(msims_or_sims, threshold=None, binning=None, sigma=None, dilate=0, device=0, keep_on_device=False):
    """Binary sample masks of the tiles: uint8 sims, 1 where the conditioned tile exceeds ``threshold``.

    Per tile, in order: block-mean ``binning`` (dict per dim, one factor, or one per dim), Gaussian smoothing with ``sigma``
    (pixels of the binned tile), the threshold (``None``: ``otsu_threshold`` of the same conditioned tiles, 256 bins),
    and a dilation by the flat box of ``2 dilate + 1`` voxels per axis (``dilate``: one radius or one per dim, at most 32; zeros
    outside the tile).  Integer tiles are compared exactly, float32 tiles against the threshold rounded to float32; a NaN is not
    sample.  The masks carry the tiles' transforms and the binned coordinates; their data is a numpy array, or stays a
    ``DeviceArray`` with ``keep_on_device``."""
    sims = _spatial_sims(msims_or_sims, "sample_masks")
    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    radius = _mask_ops.check_radius(_per_axis(dilate, sdims, "dilate"), len(sdims))
    conditioned = [_condition(s, binning, sigma, device) for s in sims]
    if threshold is None:
        threshold = _otsu_of_tiles([s.data for s in conditioned], 256, device)
    out = []
    for sim in conditioned:
        mask, _ = _mask_ops.threshold_mask(sim.data, threshold, radius, device)
        out.append(si_utils.SpatialImage(mask if keep_on_device else mask.get(), sim.dims, {d: np.asarray(sim.coords[d]) for d in sim.dims},
                                         {"transforms": dict(sim.attrs.get("transforms", {}))}))
    return out


FULL_WEIGHT = _lib.MVS_FEATHER_FULL_WEIGHT      # 252: a quarter, a half and three quarters of it are integers


def feather(mask, width, device=0, keep_on_device=False):
    """A binary mask as a feathered weight tile for ``fusion.fuse(view_weights=)``: uint8, 0 on the mask's zero voxels, rising to
    ``FULL_WEIGHT`` over ``width`` voxels, ``W = rint(252 (1 - cos(pi min(t, 1))) / 2)`` with ``t`` the distance to the nearest zero
    voxel of the mask in units of the width per axis (mvs_mask_feather; tests/mask_feather_oracle.py is its scipy restatement).

    ``mask``: a 2-D / 3-D uint8 sim (``sample_masks``), numpy array or contiguous ``DeviceArray``; nonzero means "use".  ``width``:
    one integer, one per dim or a dict naming every dim, each 1..32 voxels of the mask; the one number 0 means no feather (the
    tile is 0 / ``FULL_WEIGHT``).  Voxels outside the array do not count as zero -- the tile's border is the business of the
    blending weights -- and a mask without a zero gives ``FULL_WEIGHT`` everywhere.  A sim comes back as a sim with the mask's
    coords and transforms; the data is a numpy array, or stays a ``DeviceArray`` with ``keep_on_device``."""
    is_sim = isinstance(mask, si_utils.SpatialImage) or msi_utils.is_msim(mask)
    sim = _spatial_sim(mask, "feather") if is_sim else None
    data = sim.data if is_sim else mask
    if not is_device_array(data):
        data = np.asarray(data)
    if len(data.shape) not in (2, 3):
        raise ValueError("feather: masks are 2-D or 3-D")
    sdims = si_utils.get_spatial_dims_from_sim(sim) if is_sim else ["z", "y", "x"][3 - len(data.shape):]
    widths = _mask_ops.check_feather_width(width if np.ndim(width) == 0 and not isinstance(width, dict) else _per_axis(width, sdims, "width"), len(sdims))
    if np.dtype(data.dtype) != np.uint8:
        raise TypeError(f"feather: masks are uint8, not {data.dtype}")
    if is_device_array(data) and not data.is_contiguous():
        raise TypeError("feather needs a contiguous device mask")
    out = _mask_ops.feather(data, widths, device, out_on_device=keep_on_device)
    if not is_sim:
        return out
    return si_utils.SpatialImage(out, sim.dims, {d: np.asarray(sim.coords[d]) for d in sim.dims}, {"transforms": dict(sim.attrs.get("transforms", {}))})


def fuse_labels(mask_sims, transform_key, spacing=None, device=0, output_on_backend=False):
    """The label image of the masks under ``transform_key``: an int32 sim on the grid of
    ``fusion.calc_fusion_stack_properties`` (``spacing``: dict per dim, default the first mask's) whose voxels hold the minimum,
    over the views ``i`` that cover them, of ``mask_i ? i + 1 : 0`` sampled at interpolation order 0, and 0 where no view does --
    the reference's ``fuse(mask_i * (i + 1), fusion_func=nanmin, interpolation_order=0)`` after its ``nan_to_num``
    (mvs_label_fuse; the pixel affines are derived as ``fusion.fuse_np`` derives them).  The result carries the identity under
    ``transform_key`` and the number of views as ``attrs["n_labels"]``."""
    sims = _spatial_sims(mask_sims, "fuse_labels")
    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    ndim = len(sdims)
    params = [param_utils.select_time(si_utils.get_affine_from_sim(s, transform_key), 0) for s in sims]
    if spacing is None:
        spacing = si_utils.get_spacing_from_sim(sims[0])
    spacing = {d: float(v) for d, v in zip(sdims, _per_axis(spacing, sdims, "spacing"))}
    osp = fusion.calc_fusion_stack_properties(sims, params, spacing, mode="union")
    matrices, offsets = get_pixel_affines(
        np.linalg.inv(np.stack(params)), np.stack([si_utils.get_origin_from_sim(s, asarray=True) for s in sims]),
        np.stack([si_utils.get_spacing_from_sim(s, asarray=True) for s in sims]), np.array([osp["origin"][d] for d in sdims]),
        np.array([osp["spacing"][d] for d in sdims]))
    data = _mask_ops.fuse_labels([s.data for s in sims], matrices, offsets, [osp["shape"][d] for d in sdims], device, output_on_backend)
    res = si_utils.to_spatial_image(data, dims=sdims, scale=osp["spacing"], translation=osp["origin"])
    si_utils.set_sim_affine(res, param_utils.identity_transform(ndim), transform_key)
    res.attrs["n_labels"] = len(sims)
    return res


def pairs_from_counts(counts):
    """The sorted pairs ``(i, j)``, ``i < j``, of 0-based indices with ``counts[i, j] > 0`` (the upper triangle of a contact matrix)."""
    counts = np.asarray(counts)
    i, j = np.nonzero(np.triu(counts, 1))
    return [(int(a), int(b)) for a, b in zip(i, j)]


def contact_pairs(labels, connectivity=None, return_counts=False, device=0, n_labels=None):
    """The pairs of labels of a 2-D / 3-D int32 label image that touch, as sorted 0-based ``(i, j)``, ``i < j`` (label - 1: view
    indices for the labels of ``fuse_labels``); with ``return_counts`` also the number of voxel contacts of every pair.

    ``labels``: a label sim (``fuse_labels``), a numpy array or a contiguous ``DeviceArray``.  Two voxels touch when they differ by
    at most one step on up to ``connectivity`` axes (default: all of them, the full 8- / 26-neighbourhood); background (0) touches
    nothing.  ``n_labels``: the largest label, at most 2048 (default: ``attrs["n_labels"]`` of a sim, else the maximum of a host
    array; required for a bare ``DeviceArray``)."""
    data = labels.data if isinstance(labels, si_utils.SpatialImage) else labels
    if n_labels is None and isinstance(labels, si_utils.SpatialImage):
        n_labels = labels.attrs.get("n_labels")
    if n_labels is None:
        if is_device_array(data):
            raise ValueError("contact_pairs: n_labels is required for a DeviceArray without a label sim around it")
        n_labels = max(int(np.max(data)), 1) if np.size(data) else 1
    n_labels = _mask_ops.check_n_labels(n_labels)
    if not is_device_array(data):
        data = np.asarray(data)
        if data.dtype != np.int32:
            if not np.issubdtype(data.dtype, np.integer):
                raise TypeError(f"label images are integers, not {data.dtype}")
            data = data.astype(np.int32)
    counts = _mask_ops.label_contacts(data, n_labels, connectivity, device)
    pairs = pairs_from_counts(counts)
    if return_counts:
        return pairs, np.array([counts[i, j] for i, j in pairs], dtype=np.uint64)
    return pairs
