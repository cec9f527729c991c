"""Registration quality metrics on the HIP backend (mirror of the reference's metrics.py).

``tile_pair_image_metrics`` compares the image content of adjacent views in their overlap under one or more candidate
transforms.  The geometry (overlap polytope, comparison box, halfspaces, output grid) is host algebra in float64 that restates
src/multiview_stitcher/metrics.py and registration._get_overlap_bboxes; the voxel work -- sampling both tiles on the grid,
masking and the sums of the NCC -- runs in one kernel per pair (mvs_pair_moments, csrc/mvs_pair_metrics.hip) that writes no
volume.  Metric functions other than the built-in NCC get the resampled float32 arrays the reference gives them."""

from __future__ import annotations

import logging

import numpy as np

from . import _metric_ops, msi_utils, mv_graph, param_utils
from . import spatial_image_utils as si_utils
from .transformation import get_pixel_affine, resample_array, transform_pts

logger = logging.getLogger(__name__)

# the halfspaces of an overlap are pushed outwards by this fraction of the smallest fixed spacing (metrics.py:627-630)
HALFSPACE_EXPANSION = 1e-3


def normalized_cross_correlation(im1, im2):
    """Normalised cross-correlation of two arrays of one shape (metrics.py:42-79): positions where either array is NaN are left
    out; NaN with fewer than two positions left or when either image is constant there (``sqrt(sum a_c^2 sum b_c^2) < 1e-10``).
    Host function on arrays, two-pass float64 like the reference.  As a value of ``metric_funcs`` it selects the moments kernel
    of ``tile_pair_image_metrics`` instead of being called."""
    a = np.asarray(im1, dtype=np.float64)
    b = np.asarray(im2, dtype=np.float64)
    mask = ~(np.isnan(a) | np.isnan(b))
    if np.sum(mask) < 2:
        return np.nan
    a = a[mask]
    b = b[mask]
    a_c = a - a.mean()
    b_c = b - b.mean()
    denom = np.sqrt(np.sum(a_c ** 2) * np.sum(b_c ** 2))
    if denom < 1e-10:
        return np.nan
    return float(np.dot(a_c, b_c) / denom)


def _is_builtin_ncc(func):
    """This module's NCC, or the reference's under its own name (the way fusion maps the reference's built-in functions)."""
    return func is normalized_cross_correlation or (
        getattr(func, "__name__", None) == "normalized_cross_correlation" and getattr(func, "__module__", None) == "multiview_stitcher.metrics")


def _tolerance(max_tolerance, sdims):
    """metrics.py:171-178: the (negative) amount every view box is extended by."""
    if max_tolerance is None:
        return None
    if isinstance(max_tolerance, (int, float)):
        return -float(max_tolerance)
    return {dim: -float(max_tolerance.get(dim, 0.0)) for dim in sdims}


def _affine(sim, key):
    return param_utils.select_time(si_utils.get_affine_from_sim(sim, key), 0)


def _sim_t0(msim, scale_key, metric_channel):
    """The first time point and the chosen channel of one view (metrics.py:575-588)."""
    sim = msi_utils.get_sim_from_msim(msim, scale=scale_key)
    sel = {}
    if "t" in sim.dims:
        sel["t"] = sim.coords["t"][0]
    if "c" in sim.dims:
        sel["c"] = sim.coords["c"][0] if metric_channel is None else metric_channel
    return si_utils.sim_sel_coords(sim, sel) if sel else sim


def transform_halfspace_equations(equations, affine):
    """mv_graph.transform_halfspace (mv_graph.py:258-298) on the equations alone: rows [n, c] that hold in space A, and
    ``affine`` that maps points of A to B, give ``equations @ inv(affine)`` in B."""
    return np.asarray(equations, dtype=np.float64) @ np.linalg.inv(affine)


def _overlap_geometry(sim_fixed, sim_moving, base_transform_key, tol):
    """registration._get_overlap_bboxes(sim_fixed, sim_moving, base_transform_key, None, tol) of the reference (registration.py:
    194-277) for the fixed view: the two view boxes, extended by ``tol``, are intersected as halfspaces in the world of the base
    key (the general sequence of mv_graph.get_overlap_between_pair_of_stack_props, also for axis-aligned views); the comparison
    box is the extent of the polytope's vertices in the fixed view's intrinsic space and the halfspaces are brought there too.
    No intersection: box and halfspaces are None."""
    sims = [sim_fixed, sim_moving]
    affines = [_affine(s, base_transform_key) for s in sims]
    sps = [si_utils.get_stack_properties_from_sim(s) for s in sims]
    if tol is not None:
        sps = [mv_graph.extend_stack_props(sp, tol) for sp in sps]
    vol, hs = mv_graph.get_overlap_between_pair_of_stack_props(dict(sps[0], transform=affines[0]), dict(sps[1], transform=affines[1]),
                                                               closed_form=False)
    if hs is None:
        return {"comparison_bbox": None, "halfspaces": None, "vol": float(vol)}
    to_intrinsic = np.linalg.inv(affines[0])
    boxes = [mv_graph._axis_aligned_box(dict(sp, transform=a)) for sp, a in zip(sps, affines)]
    if boxes[0] is not None and boxes[1] is not None:
        # two axis-aligned views (every stage-positioned mosaic): the polytope is the intersection of the two boxes, whose corners
        # are known exactly, where Qhull's vertices are off by a few ulp -- enough to move the floor() of the grid shape by one
        lo, hi = np.maximum(boxes[0][0], boxes[1][0]), np.minimum(boxes[0][1], boxes[1][1])
        vertices = np.array(list(np.ndindex(*([2] * len(lo))))) * (hi - lo) + lo
    else:
        vertices = np.asarray(hs.intersections)
    corners = transform_pts(vertices, to_intrinsic)
    lower, upper = np.min(corners, axis=0), np.max(corners, axis=0)
    bbox = None if np.any(lower >= upper) else {"lower": lower, "upper": upper}
    return {"comparison_bbox": bbox, "halfspaces": transform_halfspace_equations(hs.halfspaces, to_intrinsic), "vol": float(vol)}


def _graph_nodes(g):
    nodes = g.nodes
    return list(nodes() if callable(nodes) else nodes)


def _graph_edges(g):
    edges = g.edges
    return [tuple(e[:2]) for e in (edges() if callable(edges) else edges)]


def _edge_transform(g, i, j):
    """``g.edges[i, j]["transform"]`` of a networkx graph, or the attribute of this package's ``mv_graph.Graph``."""
    if isinstance(g, mv_graph.Graph):
        t = g.adj[i][j]["transform"]
    else:
        t = g.edges[i, j]["transform"]
    if hasattr(t, "coords") and "t" in getattr(t, "coords", {}):
        t = t.isel(t=0)
    return param_utils.select_time(np.asarray(getattr(t, "data", t), dtype=np.float64), 0).squeeze()


def _in_digraph_order(edges, nodes):
    """The directed edges in the order networkx.DiGraph.edges() reports them: by source node in node order, a node's edges in the
    order they were added."""
    pos = {n: k for k, n in enumerate(nodes)}
    return sorted(edges, key=lambda e: pos[e[0][0]])


def _build_metrics_edges(msims, sims_t0, base_transform_key, query_transform_keys, tol, bidirectional):
    """metrics._build_metrics_graph (metrics.py:127-246): the directed edges of Mode 1 in the reference's order, each with its
    comparison box, halfspaces, overlap volume and the transform fixed-intrinsic -> moving-intrinsic per query key.  The pairs are
    the edges of the view adjacency graph of the finest level (mv_graph.py:73-97)."""
    sims0 = [_sim_t0(msim, "scale0", None) for msim in msims]
    views = [dict(si_utils.get_stack_properties_from_sim(s), transform=_affine(s, base_transform_key)) for s in sims0]
    g_adj = mv_graph.build_view_adjacency_graph(views, overlap_tolerance=tol)
    edges = []
    for i, j in g_adj.edges():
        directions = [(i, j), (j, i)] if bidirectional else [(min(i, j), max(i, j))]
        for fixed_idx, moving_idx in directions:
            sim_fixed, sim_moving = sims_t0[fixed_idx], sims_t0[moving_idx]
            geo = _overlap_geometry(sim_fixed, sim_moving, base_transform_key, tol)
            geo["transforms"] = {q: np.linalg.inv(_affine(sim_moving, q)) @ _affine(sim_fixed, q) for q in query_transform_keys}
            edges.append(((fixed_idx, moving_idx), geo))
    return _in_digraph_order(edges, g_adj.nodes)


def _build_metrics_edges_from_pairs_graph(sims_t0, base_transform_key, pairs_graph, tol, bidirectional):
    """metrics._build_metrics_graph_from_pairs_graph (metrics.py:249-379): Mode 2.  The edge attribute ``"transform"`` maps the
    world of the lower-index view to the world of the higher-index view; the reverse direction keeps the reference's expression
    (metrics.py:365-368) as it stands."""
    edges = []
    for i, j in _graph_edges(pairs_graph):
        fixed_base, moving_base = min(i, j), max(i, j)
        T_edge = _edge_transform(pairs_graph, fixed_base, moving_base)
        directions = [(fixed_base, moving_base), (moving_base, fixed_base)] if bidirectional else [(fixed_base, moving_base)]
        for fixed_idx, moving_idx in directions:
            sim_fixed, sim_moving = sims_t0[fixed_idx], sims_t0[moving_idx]
            geo = _overlap_geometry(sim_fixed, sim_moving, base_transform_key, tol)
            T_fixed_base, T_moving_base = _affine(sim_fixed, base_transform_key), _affine(sim_moving, base_transform_key)
            if fixed_idx < moving_idx:
                p_moving = np.linalg.inv(T_moving_base) @ T_edge @ T_fixed_base
            else:
                p_moving = np.linalg.inv(T_fixed_base) @ np.linalg.inv(T_edge) @ T_moving_base
            geo["transforms"] = {"transform": p_moving}
            edges.append(((fixed_idx, moving_idx), geo))
    return _in_digraph_order(edges, _graph_nodes(pairs_graph))


def comparison_grid(bbox, spacing):
    """The output grid of one pair (metrics.py:685-706): origin = the box's lower corner, ``shape = max(1, floor((upper - lower) /
    spacing + 1))`` per axis.  ``spacing``: float64 array in axis order."""
    lower, upper = np.asarray(bbox["lower"], dtype=np.float64), np.asarray(bbox["upper"], dtype=np.float64)
    shape = tuple(max(1, int(np.floor((upper[k] - lower[k]) / spacing[k] + 1))) for k in range(len(lower)))
    return np.array([float(v) for v in lower]), shape


def halfspaces_to_grid_index(equations, origin, spacing):
    """Rows [n, c] over physical coordinates ``x = origin + spacing * index`` as rows [a, b] over the index: ``a = n * spacing``,
    ``b = n . origin + c``."""
    equations = np.asarray(equations, dtype=np.float64)
    normals, c = equations[:, :-1], equations[:, -1]
    return np.concatenate([normals * spacing[None, :], (normals @ origin + c)[:, None]], axis=1)


def halfspace_mask(grid_equations, shape):
    """True where ``((a_z z + a_y y) + a_x x) + b <= 0`` holds for every row, over the index grid of ``shape`` -- the arithmetic
    of the kernel's mask, in float64."""
    ndim = len(shape)
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    mask = np.ones(shape, dtype=bool)
    for row in np.asarray(grid_equations, dtype=np.float64).reshape(-1, ndim + 1):
        v = row[0] * idx[0]
        for k in range(1, ndim):
            v = v + row[k] * idx[k]
        mask &= (v + row[ndim]) <= 0
    return mask


def _pair_metrics(sim_fixed, sim_moving, geo, candidate_keys, spacing_d, fixed_spacing_t0, metric_funcs, device):
    """The metrics of one directed pair with a comparison box, for every candidate key."""
    sdims = si_utils.get_spatial_dims_from_sim(sim_fixed)
    ndim = len(sdims)
    spacing = np.array([float(spacing_d[d]) for d in sdims])
    origin, shape = comparison_grid(geo["comparison_bbox"], spacing)
    equations = np.array(geo["halfspaces"], dtype=np.float64)
    equations[:, -1] -= HALFSPACE_EXPANSION * np.min(fixed_spacing_t0)          # mv_graph.expand_halfspace (mv_graph.py:244-246)
    grid_eqs = halfspaces_to_grid_index(equations, origin, spacing)
    # grid index -> pixel of either tile: the parameters transform_sim derives (transformation.py:37-83)
    fixed_affine = get_pixel_affine(np.eye(ndim + 1), si_utils.get_origin_from_sim(sim_fixed, asarray=True),
                                    si_utils.get_spacing_from_sim(sim_fixed, asarray=True), origin, spacing)
    cand_affines = [get_pixel_affine(geo["transforms"][q], si_utils.get_origin_from_sim(sim_moving, asarray=True),
                                     si_utils.get_spacing_from_sim(sim_moving, asarray=True), origin, spacing) for q in candidate_keys]
    out = {q: {} for q in candidate_keys}
    if any(_is_builtin_ncc(f) for f in metric_funcs.values()):
        moments = _metric_ops.pair_moments(sim_fixed.data, sim_moving.data, fixed_affine, cand_affines, shape, grid_eqs, device)
        ncc = [_metric_ops.ncc_from_moments(m) for m in moments]
    others = {k: f for k, f in metric_funcs.items() if not _is_builtin_ncc(f)}
    if others:
        # what the reference hands a metric function (metrics.py:111-124): float32 arrays, NaN outside either tile, the fixed one
        # also NaN outside the halfspaces
        fixed_np = np.array(resample_array(sim_fixed.data, fixed_affine[0], fixed_affine[1], shape, order=1, cval=np.nan, device=device,
                                           out_on_device=False), dtype=np.float32)
        fixed_np[~halfspace_mask(grid_eqs, shape)] = np.nan
    for iq, q in enumerate(candidate_keys):
        if others:
            moving_np = np.asarray(resample_array(sim_moving.data, cand_affines[iq][0], cand_affines[iq][1], shape, order=1, cval=np.nan,
                                                  device=device, out_on_device=False), dtype=np.float32)
        for key, func in metric_funcs.items():
            out[q][key] = ncc[iq] if _is_builtin_ncc(func) else float(func(fixed_np, moving_np))
    return out


def summarize(pair_values, volumes, candidate_keys, metric_keys):
    """Overlap-volume-weighted mean per candidate key and metric key over the directed pairs (metrics.py:773-794): NaN values are
    left out of numerator and denominator; NaN when none is left."""
    summary = {}
    for q in candidate_keys:
        summary[q] = {}
        for metric_key in metric_keys:
            valid = [(float(pair_values[p][q].get(metric_key, np.nan)), float(volumes[p])) for p in pair_values]
            valid = [(v, w) for v, w in valid if not np.isnan(v)]
            total_w = sum(w for _, w in valid)
            summary[q][metric_key] = float(sum(v * w for v, w in valid) / total_w) if valid and total_w > 0 else np.nan
    return summary


def tile_pair_image_metrics(
    msims,
    base_transform_key,
    query_transform_keys=None,
    metric_funcs=None,
    max_tolerance=None,
    spacing=None,
    bidirectional=False,
    metric_channel=None,
    n_parallel_pairs=None,
    input_res_level=None,
    *,
    pairs_graph=None,
    device=0,
):
    """metrics.tile_pair_image_metrics (metrics.py:387-808) on the HIP backend: registration quality metrics of the overlapping
    pairs of ``msims``.

    Exactly one of ``query_transform_keys`` (Mode 1: pairs from the overlap of the views under ``base_transform_key``, metrics
    under every query key) and ``pairs_graph`` (Mode 2: pairs and their world-space ``"transform"`` from a pairwise registration
    graph -- ``mv_graph.Graph`` or networkx -- with the single candidate key ``"transform"``) is given.  Per directed pair the
    comparison box is the extent, in the fixed view's intrinsic space, of the intersection of the two view boxes shrunk by
    ``max_tolerance`` (float, or dict per dim); both tiles are sampled linearly on the grid of ``spacing`` (dict; default: the
    fixed view's) over that box, the moving one through ``inv(T_moving_q) @ T_fixed_q``, and samples outside the (slightly
    expanded) intersection polytope do not count.  ``input_res_level`` / ``spacing`` choose the resolution level as in the
    reference; only the first time point is used, and ``metric_channel`` (a channel coordinate) or the first channel.

    ``metric_funcs`` maps names to ``func(im1, im2) -> float``; default ``{"ncc": normalized_cross_correlation}``.  The built-in
    NCC (this module's, or the reference's) is computed by one gather-and-reduce kernel per pair without materialising any array;
    every other function receives float32 arrays with NaN outside the tiles and, in the fixed one, outside the polytope.

    ``n_parallel_pairs`` is accepted for compatibility and ignored: the pairs run one after the other on the stream of the
    context ``device``.  Tiles may be numpy arrays or ``DeviceArray``s; resident tiles are read in place.

    Returns ``{"pairs": {(fixed, moving): {candidate_key: {metric_key: float}}}, "bboxes": {(fixed, moving): {"lower", "upper"} or
    None}, "summary": {candidate_key: {metric_key: overlap-volume-weighted mean over the pairs, NaN values left out}}}``.  A pair
    without a comparison box keeps its entries, with NaN metrics."""
    if (query_transform_keys is None) == (pairs_graph is None):
        raise ValueError("Exactly one of 'query_transform_keys' or 'pairs_graph' must be provided.")
    if metric_funcs is None:
        metric_funcs = {"ncc": normalized_cross_correlation}
    if query_transform_keys is not None:
        if isinstance(query_transform_keys, str):
            query_transform_keys = [query_transform_keys]
        candidate_keys = list(query_transform_keys)
    else:
        candidate_keys = ["transform"]

    # metrics.py:557-570: a level per pair only when a spacing is given without a level
    per_pair_res_level = False
    if input_res_level is None:
        if spacing is None:
            input_res_level = 0
        else:
            per_pair_res_level = True
    graph_scale_key = "scale0" if per_pair_res_level else f"scale{input_res_level}"
    sims_t0 = [_sim_t0(msim, graph_scale_key, metric_channel) for msim in msims]
    sdims = si_utils.get_spatial_dims_from_sim(sims_t0[0])
    tol = _tolerance(max_tolerance, sdims)

    if query_transform_keys is not None:
        edges = _build_metrics_edges(msims, sims_t0, base_transform_key, candidate_keys, tol, bidirectional)
    else:
        edges = _build_metrics_edges_from_pairs_graph(sims_t0, base_transform_key, pairs_graph, tol, bidirectional)

    computed, bboxes, volumes = {}, {}, {}
    for pair, geo in edges:
        fixed_idx, moving_idx = pair
        bboxes[pair], volumes[pair] = geo["comparison_bbox"], geo["vol"]
        if geo["comparison_bbox"] is None:
            logger.warning("Empty comparison bbox for directed pair (%s -> %s), all metrics will be NaN.", fixed_idx, moving_idx)
            computed[pair] = {q: {k: np.nan for k in metric_funcs} for q in candidate_keys}
            continue
        if per_pair_res_level:
            scale_key = f"scale{msi_utils.get_res_level_from_spacing(msims[fixed_idx], spacing)}"
            sim_fixed, sim_moving = (_sim_t0(msims[i], scale_key, metric_channel) for i in pair)
        else:
            sim_fixed, sim_moving = sims_t0[fixed_idx], sims_t0[moving_idx]
        spacing_d = spacing if spacing is not None else si_utils.get_spacing_from_sim(sim_fixed)
        computed[pair] = _pair_metrics(sim_fixed, sim_moving, geo, candidate_keys, spacing_d,
                                       si_utils.get_spacing_from_sim(sims_t0[fixed_idx], asarray=True), metric_funcs, device)

    return {
        "pairs": {pair: {q: computed[pair][q] for q in candidate_keys} for pair, _ in edges},
        "bboxes": {pair: bboxes[pair] for pair, _ in edges},
        "summary": summarize(computed, volumes, candidate_keys, list(metric_funcs)),
    }
