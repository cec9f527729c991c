"""Stitching per-tile segmentations into one label image on the GPU.

Large mosaics are segmented tile by tile; the result is one integer label tile per view, with ids that mean nothing outside their
tile.  This module brings them across: the voxel count of every label (``label_counts``), the co-occurrence table of the labels
of every pair of overlapping tiles (``pair_overlaps``), the matching of labels across tiles into objects on the host
(``match_labels``: union-find over the pairs whose overlap score reaches a threshold) and the fusion of the tiles through the
resulting look-up tables, the interior-most view deciding (``fuse_label_tiles``).  ``stitch_labels`` runs the four in sequence.

All voxel work runs in HIP kernels (csrc/mvs_labels.hip; include/mvs_hip.h states their rules and limits); every result is an
integer, so equal inputs give equal bits.  2-D and 3-D; label tiles of any integer dtype in host memory (converted to int32; a value
above 2^31 - 1 raises ValueError) or resident int32 ``DeviceArray``s (strided windows with contiguous rows are fine); negative
labels are background.  Label sims with ``t`` or ``c`` dims raise NotImplementedError: one spatial label tile per view.
``masks.fuse_labels`` is a different tool: it paints the *view indices* of binary masks for pair selection.

Where the segmentations come from a threshold, they are made here too: ``label_components`` turns every thresholded tile into
objects (connected components with the numbering of ``scipy.ndimage.label``; csrc/mvs_components.hip), so a mosaic goes from
images to one label image in three calls without a voxel leaving the device::

    threshold = masks.otsu_threshold(msims, device=0)
    tiles = labels.label_components(msims, threshold, connectivity=1, min_voxels=20, keep_on_device=True)
    objects = labels.stitch_labels(tiles, "registered", output_on_backend=True)

Objects that span tiles are ``stitch_labels``' business: ``label_components`` knows one tile at a time.
"""

from __future__ import annotations

import numpy as np

from . import _label_ops, fusion, msi_utils, param_utils
from . import spatial_image_utils as si_utils
from .transformation import get_pixel_affine, get_pixel_affines


def _label_sims(label_sims, who, param="label_sims", kind="label"):
    """The full-resolution spatial label images of the views; ``t`` / ``c`` dims are refused under the parameter's name."""
    sims = []
    for i, image in enumerate(label_sims):
        sim = msi_utils.get_sim_from_msim(image, scale="scale0") if msi_utils.is_msim(image) else image
        for d in sim.dims:
            if d in ("t", "c"):
                raise NotImplementedError(f"{who}: {param}[{i}] has a {d!r} dim; per-time-point / per-channel {kind} tiles are not supported "
                                          f"(one spatial {kind} tile per view)")
        if len(si_utils.get_spatial_dims_from_sim(sim)) not in (2, 3):
            raise ValueError(f"{who}: {kind} sims are 2-D or 3-D")
        sims.append(sim)
    if not sims:
        raise ValueError(f"{who}: no tiles")
    if len({tuple(si_utils.get_spatial_dims_from_sim(s)) for s in sims}) != 1:
        raise ValueError(f"{who}: the {kind} sims differ in their spatial dims")
    return sims


def _affine(sim, transform_key):
    return np.asarray(param_utils.select_time(si_utils.get_affine_from_sim(sim, transform_key), 0), dtype=np.float64)


def label_components(images, threshold=None, connectivity=1, min_voxels=1, device=0, keep_on_device=False):
    """Per view the int32 label sim of the connected components of its thresholded tile (mvs_label_components): the objects of one
    tile, ready for ``stitch_labels(..., transform_key)``.

    ``images``: sims or msims (scale0) -- uint8 / uint16 / float32 image tiles, or the uint8 masks of ``masks.sample_masks`` on the
    tiles' own grids; host data or ``DeviceArray``s.  A voxel is foreground when ``(float32)v > (float32)threshold``: ``threshold``
    is ROUNDED TO FLOAT32 before the comparison, a voxel equal to it and a NaN are background.  ``threshold``: one number, or one per
    view; ``None`` requires uint8 tiles and means 0.  ``connectivity`` ``1 .. ndim`` is the neighbourhood of
    ``scipy.ndimage.generate_binary_structure(ndim, connectivity)``; components with fewer than ``min_voxels`` voxels become
    background.  Ids are ``1 .. n`` in ascending raster order of each component's first voxel -- the numbering of
    ``scipy.ndimage.label`` -- and ``attrs["n_labels"]`` holds ``n``.

    Every result has its source's dims, origin, spacing and every transform the source carries.  Its data is a numpy array, or a
    resident ``DeviceArray`` with ``keep_on_device`` or when the source's is one.  Sims with ``t`` / ``c`` dims raise
    NotImplementedError."""
    sims = _label_sims(images, "label_components", param="images", kind="image")
    thresholds = [threshold] * len(sims) if threshold is None or np.ndim(threshold) == 0 else list(threshold)
    if len(thresholds) != len(sims):
        raise ValueError(f"label_components: threshold: one number, or one per view ({len(sims)}), not {len(thresholds)}")
    out = []
    for sim, thr in zip(sims, thresholds):
        data, n = _label_ops.label_components(sim.data, thr, connectivity=connectivity, min_voxels=min_voxels, device=device, out_on_device=keep_on_device)
        sdims = si_utils.get_spatial_dims_from_sim(sim)
        res = si_utils.to_spatial_image(data, dims=sdims, scale=si_utils.get_spacing_from_sim(sim), translation=si_utils.get_origin_from_sim(sim))
        for key in si_utils.get_tranform_keys_from_sim(sim):
            si_utils.set_sim_affine(res, si_utils.get_affine_from_sim(sim, key), key)
        res.attrs["n_labels"] = n
        out.append(res)
    return out


def label_counts(label_sims, device=0):
    """Per view the uint64 array ``n[l]`` of the voxels with label ``l``, ``l = 0 .. max label of the view`` (mvs_label_counts).
    Negative labels are background and count as 0."""
    return [_label_ops.label_counts(s.data, device) for s in _label_sims(label_sims, "label_counts")]


def view_pairs(sims, transform_key):
    """The edges of the overlap graph of the views as ``register()`` builds it, without pruning: sorted ``(a, b)``, ``a < b``."""
    from . import mv_graph

    views = [dict(si_utils.get_stack_properties_from_sim(s), transform=_affine(s, transform_key)) for s in sims]
    g = mv_graph.build_view_adjacency_graph(views, overlap_tolerance=None)
    return sorted({(min(int(i), int(j)), max(int(i), int(j))) for i, j in g.edges()})


def footprint_box(matrix, offset, shape_a, shape_b):
    """``(lo, n)``: the integer box of tile ``a`` that bounds the footprint of tile ``b``, where ``matrix`` / ``offset`` map a pixel
    index of ``a`` to a pixel coordinate of ``b``: the corners of ``[0, n_b - 1]`` mapped back, one voxel of margin, clipped to
    ``a``.  ``n`` has a zero where the footprint misses ``a``; a singular matrix gives the whole tile.  (The kernel tests every
    voxel of the box: it only has to be large enough.)"""
    shape_a, shape_b = np.asarray(shape_a, dtype=np.int64), np.asarray(shape_b, dtype=np.int64)
    ndim = len(shape_a)
    try:
        inv = np.linalg.inv(np.asarray(matrix, dtype=np.float64))
    except np.linalg.LinAlgError:
        return [0] * ndim, [int(n) for n in shape_a]
    corners = np.array(list(np.ndindex(*([2] * ndim))), dtype=np.float64) * (shape_b - 1)
    back = (corners - np.asarray(offset, dtype=np.float64)) @ inv.T
    if not np.all(np.isfinite(back)):
        return [0] * ndim, [int(n) for n in shape_a]
    lo = np.maximum(np.floor(back.min(axis=0)) - 1, 0)
    hi = np.minimum(np.ceil(back.max(axis=0)) + 1, shape_a - 1)
    return [int(v) for v in lo], [int(max(h - l + 1, 0)) for l, h in zip(lo, hi)]


def pair_geometry(sim_a, sim_b, transform_key):
    """``(matrix, offset, box_lo, box_n)`` of the directed pair ``(a, b)``: the map from a pixel index of ``a`` to a pixel coordinate
    of ``b`` through the two views' affines under ``transform_key`` and their origins and spacings (``get_pixel_affine`` with
    ``a``'s grid as the output grid), and the box of ``a`` that bounds ``b``'s footprint."""
    p = np.linalg.inv(_affine(sim_b, transform_key)) @ _affine(sim_a, transform_key)
    matrix, offset = get_pixel_affine(p, si_utils.get_origin_from_sim(sim_b, asarray=True), si_utils.get_spacing_from_sim(sim_b, asarray=True),
                                      si_utils.get_origin_from_sim(sim_a, asarray=True), si_utils.get_spacing_from_sim(sim_a, asarray=True))
    lo, n = footprint_box(matrix, offset, sim_a.data.shape, sim_b.data.shape)
    return matrix, offset, lo, n


def pair_overlaps(label_sims, transform_key, pairs=None, device=0):
    """The co-occurrence tables of the overlapping pairs of label tiles: a dict ``{(a, b): (la, lb, n)}`` with ``a < b`` and three
    arrays (int32, int32, uint64) sorted lexicographically by ``(la, lb)`` (mvs_label_pair_overlaps).

    ``n[i]`` counts the voxels ``p`` of tile ``a``'s own pixel grid at which tile ``b`` is in bounds (``0 <= c <= n - 1`` on every
    axis, ``c`` the pixel coordinate of ``p`` in ``b``) with ``max(A[p], 0) == la[i]`` and ``max(B[floor(c + 0.5)], 0) == lb[i]``;
    the entry ``(0, 0)`` is left out, rows with one zero label are part of the table (they carry the marginals).  ``pairs``: the
    ``(i, j)`` to use (default: the edges of the overlap graph as ``register()`` builds it, without pruning); each undirected pair
    is used once, the lower index as ``a``."""
    sims = _label_sims(label_sims, "pair_overlaps")
    if pairs is None:
        pairs = view_pairs(sims, transform_key)
    pairs = sorted({(min(int(i), int(j)), max(int(i), int(j))) for i, j in pairs})
    if any(a == b or a < 0 or b >= len(sims) for a, b in pairs):
        raise ValueError("pairs: two different view indices each")
    tables = {}
    for a, b in pairs:
        matrix, offset, lo, n = pair_geometry(sims[a], sims[b], transform_key)
        tables[(a, b)] = _label_ops.pair_overlaps(sims[a].data, sims[b].data, matrix, offset, lo, n, device)
    return tables


def _marginal(labels, n):
    """Per row the sum of ``n`` over the rows with the same label (float64; exact below 2^53)."""
    _, inverse = np.unique(labels, return_inverse=True)
    return np.bincount(inverse.reshape(-1), weights=n)[inverse.reshape(-1)]


def match_labels(counts, overlaps, criterion="iou", threshold=0.5, min_voxels=1):
    """Match the labels of the tiles into objects.  Host only, float64: touches no device.

    ``counts``: per view the array of ``label_counts``; ``overlaps``: the dict of ``pair_overlaps``.  Within one pair, with
    ``A_ov(la)`` and ``B_ov(lb)`` the sums of the table over ``lb`` and over ``la`` (the rows with a zero label included), the rows
    with ``la, lb > 0`` and ``n >= min_voxels`` score ``n / (A_ov + B_ov - n)`` (``"iou"``) or ``n / min(A_ov, B_ov)``
    (``"min_fraction"``), and an edge joins ``(a, la)`` and ``(b, lb)`` when the score is ``>= threshold``.  The nodes are all
    ``(view, label)`` with ``label > 0`` and a non-zero count; the objects are the connected components, numbered ``1 ..
    n_objects`` in ascending order of their smallest ``(view, label)`` member.

    Returns ``(luts, n_objects)``: per view an int32 look-up table of length ``max label + 1`` with ``lut[0] == 0`` (and 0 for the
    labels without a voxel)."""
    if criterion not in ("iou", "min_fraction"):
        raise ValueError(f"criterion must be 'iou' or 'min_fraction', not {criterion!r}")
    counts = [np.asarray(c).reshape(-1) for c in counts]
    if any(c.size < 1 for c in counts):
        raise ValueError("counts: every view needs at least the count of label 0")
    starts = np.concatenate([[0], np.cumsum([c.size for c in counts])]).astype(np.int64)
    parent = np.arange(starts[-1], dtype=np.int64)

    def find(i):
        root = i
        while parent[root] != root:
            root = parent[root]
        while parent[i] != root:
            parent[i], i = root, parent[i]
        return root

    for (a, b), (la, lb, n) in sorted(overlaps.items()):
        if not (0 <= a < len(counts) and 0 <= b < len(counts)) or a == b:
            raise ValueError(f"overlaps: pair {(a, b)} names no two views of counts")
        la, lb = np.asarray(la).astype(np.int64).reshape(-1), np.asarray(lb).astype(np.int64).reshape(-1)
        n = np.asarray(n).astype(np.float64).reshape(-1)
        if not la.size:
            continue
        a_ov, b_ov = _marginal(la, n), _marginal(lb, n)
        with np.errstate(divide="ignore", invalid="ignore"):
            score = n / (a_ov + b_ov - n) if criterion == "iou" else n / np.minimum(a_ov, b_ov)
        for i in np.nonzero((la > 0) & (lb > 0) & (n >= min_voxels) & (score >= threshold))[0]:
            if la[i] >= counts[a].size or lb[i] >= counts[b].size or not counts[a][la[i]] or not counts[b][lb[i]]:
                raise ValueError(f"overlaps: pair {(a, b)} names the labels {(int(la[i]), int(lb[i]))}, which counts does not")
            ra, rb = find(starts[a] + la[i]), find(starts[b] + lb[i])
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)

    # the root of a component is its smallest node (the smaller root always wins): number the roots in ascending order
    luts, ids, n_objects = [], {}, 0
    for v, c in enumerate(counts):
        lut = np.zeros(c.size, dtype=np.int32)
        for label in np.nonzero(c[1:])[0] + 1:
            root = find(starts[v] + label)
            if root not in ids:
                n_objects += 1
                ids[root] = n_objects
            lut[label] = ids[root]
        luts.append(lut)
    return luts, n_objects


def _on_grid(props, whole, sdims, tol=1e-6):
    """The integer index of the first voxel of the grid ``props`` on the grid ``whole``, or None when it is not a box of it (another
    spacing, an origin between two voxels)."""
    origin = []
    for d in sdims:
        if abs(float(props["spacing"][d]) - float(whole["spacing"][d])) > 1e-9 * abs(float(whole["spacing"][d])):
            return None
        k = (float(props["origin"][d]) - float(whole["origin"][d])) / float(whole["spacing"][d])
        if abs(k - np.round(k)) > tol:
            return None
        origin.append(int(np.round(k)))
    return origin


def fuse_label_tiles(label_sims, transform_key, luts=None, output_stack_properties=None, spacing=None, device=0, output_on_backend=False):
    """The label image of the tiles under ``transform_key``: an int32 sim on the grid of ``fusion.calc_fusion_stack_properties``
    (``spacing``: dict per dim, default the first tile's) or on ``output_stack_properties`` (``shape`` / ``spacing`` / ``origin`` per
    dim) (mvs_label_tiles_fuse).

    Per output voxel ``p``, among the views in bounds, the one with the largest ``d_v = min over the axes with n_k > 1 of
    min(c_k, (n_k - 1) - c_k)`` decides -- the interior-most view -- and ties go to the lowest view index; the voxel gets
    ``luts[w][L_w[floor(c + 0.5)]]``, and 0 where that label is negative or not below ``len(luts[w])`` or no view is in bounds.
    The winner's background wins too: seams are hard, and matched objects line up across them because they share an id.
    ``luts``: None (every view the identity) or per view a table of ``match_labels`` (or None).

    A box of the whole grid -- ``output_stack_properties`` with the whole grid's spacing and an origin on one of its voxels --
    equals the crop of the whole result bit for bit: the view parameters are derived once for the whole grid and the indices
    shifted as integers.  Any other grid is a frame of its own.  The result carries the identity under ``transform_key``; its data
    is a numpy array, or stays a ``DeviceArray`` with ``output_on_backend``."""
    sims = _label_sims(label_sims, "fuse_label_tiles")
    sdims = si_utils.get_spatial_dims_from_sim(sims[0])
    ndim = len(sdims)
    params = [_affine(s, transform_key) for s in sims]
    if spacing is None:
        spacing = output_stack_properties["spacing"] if output_stack_properties is not None else si_utils.get_spacing_from_sim(sims[0])
    if not isinstance(spacing, dict):
        spacing = dict(zip(sdims, [spacing] * ndim if np.ndim(spacing) == 0 else spacing))
    spacing = {d: float(spacing[d]) for d in sdims}
    frame = fusion.calc_fusion_stack_properties(sims, params, spacing, mode="union")
    out, origin = frame, [0] * ndim
    if output_stack_properties is not None:
        out = {k: {d: output_stack_properties[k][d] for d in sdims} for k in ("shape", "spacing", "origin")}
        origin = _on_grid(out, frame, sdims)
        if origin is None:
            frame, origin = out, [0] * ndim
    matrices, offsets = get_pixel_affines(
        np.linalg.inv(np.stack(params)), np.stack([si_utils.get_origin_from_sim(s, asarray=True) for s in sims]),
        np.stack([si_utils.get_spacing_from_sim(s, asarray=True) for s in sims]), np.array([frame["origin"][d] for d in sdims]),
        np.array([frame["spacing"][d] for d in sdims]))
    data = _label_ops.fuse_label_tiles([s.data for s in sims], matrices, offsets, luts, [int(out["shape"][d]) for d in sdims], origin, device,
                                       output_on_backend)
    res = si_utils.to_spatial_image(data, dims=sdims, scale={d: float(out["spacing"][d]) for d in sdims},
                                    translation={d: float(out["origin"][d]) for d in sdims})
    si_utils.set_sim_affine(res, param_utils.identity_transform(ndim), transform_key)
    return res


def stitch_labels(label_sims, transform_key, pairs=None, criterion="iou", threshold=0.5, min_voxels=1, output_stack_properties=None,
                  spacing=None, device=0, output_on_backend=False):
    """Per-tile segmentations as one label image: ``label_counts``, ``pair_overlaps``, ``match_labels`` and ``fuse_label_tiles`` in
    sequence.  Returns the fused int32 sim; ``attrs["n_objects"]`` is the number of objects, which carry the ids ``1 ..
    n_objects``."""
    sims = _label_sims(label_sims, "stitch_labels")
    counts = label_counts(sims, device=device)
    overlaps = pair_overlaps(sims, transform_key, pairs=pairs, device=device)
    luts, n_objects = match_labels(counts, overlaps, criterion=criterion, threshold=threshold, min_voxels=min_voxels)
    res = fuse_label_tiles(sims, transform_key, luts=luts, output_stack_properties=output_stack_properties, spacing=spacing, device=device,
                           output_on_backend=output_on_backend)
    res.attrs["n_objects"] = n_objects
    return res
