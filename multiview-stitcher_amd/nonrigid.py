"""Non-rigid tile refinement on the HIP backend: remove the doubled structures that one affine per tile leaves in the overlaps.

Stage non-linearity, field curvature and refractive distortion in cleared tissue are local; ``registration`` ends at 12 parameters
per pair and ``fusion.fuse`` blends what is left into blur.  ``fit_fields`` estimates, per view, a coarse grid of displacement
vectors from block matching in the overlaps (BigStitcher's non-rigid fusion is the model; the reference has no counterpart),
``apply_fields`` warps whole tiles by them before ``fusion.fuse``.

Model: view ``v`` has ``nodes_v = (gz, gy, gx)`` cells under the cell rule of the intensity maps (``_intensity_ops.cell_index`` /
``cell_centres``), each with one displacement ``d`` in pixels of that view (z, y, x).  The corrected tile is
``I'(p) = I(clamp(p + d(p), 0, n - 1))`` with ``d(p)`` interpolated multilinearly between the cell centres and held constant beyond
the outermost ones (``axis_table``), read with the library's linear sampler.  It keeps its grid, transforms and dtype.

The voxel work runs in two kernels (csrc/mvs_nonrigid.hip): mvs_block_match reduces every block of a pair's overlap grid to six
moments per integer shift of a search window, mvs_field_warp warps a tile.  The planner, the peak search and the solver below are
host algebra in float64.

Sign convention: if tile ``v`` shows ``G(x + e_v(x))``, block matching finds ``F(g) ~ M(g + s)`` with ``s = e_F - e_M``; the ideal
``u_v = -e_v`` then satisfies ``u_M - u_F = s``."""

from __future__ import annotations

import numpy as np

from . import _lib, _nonrigid_ops, intensity, metrics
from . import spatial_image_utils as si_utils
from ._intensity_ops import cell_index

DROP_REASONS = ("few_samples", "low_ncc", "rim", "flat")


# ---- blocks of one pair ------------------------------------------------------------------------------------------------------------
def plan_blocks(grid_shape, block, fixed_affine, moving_affine, shape_f, shape_m, nodes_f, nodes_m):
    """The blocks of one pair for mvs_block_match: an int64 array ``(B, 4, ndim)`` with the rows ``lo, n, cell_f, cell_m``.  Host
    only.

    The grid of ``grid_shape`` is tiled into boxes of at most ``block`` per axis (C order; the partial boxes at the far end are
    kept).  ``fixed_affine`` / ``moving_affine = (matrix, offset)`` map a grid index to a pixel of the tile of ``shape_f`` /
    ``shape_m``; the cell of a box in either tile is the cell rule applied to the pixel coordinate of the box centre
    ``lo + (n - 1) / 2``, clamped into the tile."""
    grid_shape = tuple(int(s) for s in grid_shape)
    ndim = len(grid_shape)
    block = (int(block),) * ndim if isinstance(block, (int, np.integer)) else tuple(int(b) for b in block)
    if len(block) != ndim or any(b < 1 for b in block):
        raise ValueError("block: a positive int, or one per axis")
    starts = [np.arange(0, s, b) for s, b in zip(grid_shape, block)]
    lo = np.array(list(np.ndindex(*[len(s) for s in starts])), dtype=np.int64).reshape(-1, ndim) * np.asarray(block, dtype=np.int64)
    n = np.minimum(np.asarray(block, dtype=np.int64), np.asarray(grid_shape, dtype=np.int64) - lo)
    centre = lo + (n - 1) / 2.0
    out = np.zeros((len(lo), 4, ndim), dtype=np.int64)
    out[:, 0], out[:, 1] = lo, n
    for row, affine, shape, nodes in ((2, fixed_affine, shape_f, nodes_f), (3, moving_affine, shape_m, nodes_m)):
        matrix, offset = np.asarray(affine[0], dtype=np.float64), np.asarray(affine[1], dtype=np.float64)
        pix = centre @ matrix.T + offset
        for ax in range(ndim):
            out[:, row, ax] = cell_index(np.clip(pix[:, ax], 0.0, shape[ax] - 1.0), int(nodes[ax]), int(shape[ax]))
    return out


# ---- shifts from moments -------------------------------------------------------------------------------------------------------------
def ncc_of_moments(moments):
    """``_metric_ops.ncc_from_moments`` over the rows of an array ``(..., 6)``: NaN with fewer than two sample pairs or when
    ``sqrt(M2_f * M2_m) < 1e-10``, else ``C_fm / sqrt(M2_f * M2_m)``."""
    m = np.asarray(moments, dtype=np.float64)
    denom = np.sqrt(m[..., 3] * m[..., 4])
    ok = (m[..., 0] >= 2) & ~(denom < 1e-10)
    return np.where(ok, m[..., 5] / np.where(ok, denom, 1.0), np.nan)


def shifts_from_moments(moments, radius, min_samples=64, min_ncc=0.3):
    """The sub-pixel shift and the weight of every block from the moments of mvs_block_match.  Host only, float64.

    ``moments``: ``(B, S, 6)``, ``S = prod (2 r + 1)``, the shift index z slowest; ``radius``: per axis.  Per block the NCC of every
    shift is that of ``_metric_ops.ncc_from_moments`` and the peak its first maximum in index order (NaNs left out; the zero shift
    when all are NaN).  The block is dropped, with the first reason that holds, when
      ``few_samples``  the ``n`` at the peak is below ``min_samples``;
      ``low_ncc``      the NCC at the peak is NaN or below ``min_ncc``;
      ``rim``          the peak lies on the rim of the window on an axis of radius > 0;
      ``flat``         on such an axis a neighbour of the peak is NaN or the second difference ``c- - 2 c0 + c+`` is not negative.
    Else, per axis, ``s = k + clip(0.5 (c- - c+) / (c- - 2 c0 + c+), -0.5, 0.5)`` with ``k`` the peak's integer shift (``s = 0`` on an
    axis of radius 0) and the weight is ``w = n * ncc``.

    Returns ``{"shift": (B, ndim) float64 (NaN where dropped), "weight": (B,), "reason": list of None / str, "ncc": (B,) the NCC
    at the peak, "n": (B,)}``."""
    radius = tuple(int(r) for r in radius)
    ndim = len(radius)
    window = tuple(2 * r + 1 for r in radius)
    m = np.asarray(moments, dtype=np.float64)
    if m.ndim != 3 or m.shape[1:] != (int(np.prod(window)), 6):
        raise ValueError("moments must have shape (B, prod (2 r + 1), 6)")
    ncc = ncc_of_moments(m)
    zero = int(np.ravel_multi_index(radius, window))
    B = len(m)
    shift = np.full((B, ndim), np.nan)
    weight = np.zeros(B)
    reason = [None] * B
    peak_ncc, peak_n = np.full(B, np.nan), np.zeros(B)
    for b in range(B):
        c = ncc[b]
        idx = int(np.nanargmax(c)) if np.any(~np.isnan(c)) else zero
        k = np.unravel_index(idx, window)
        c0, n = c[idx], m[b, idx, 0]
        peak_ncc[b], peak_n[b] = c0, n
        if n < min_samples:
            reason[b] = "few_samples"
            continue
        if np.isnan(c0) or c0 < min_ncc:
            reason[b] = "low_ncc"
            continue
        axes = [ax for ax in range(ndim) if radius[ax] > 0]
        if any(k[ax] == 0 or k[ax] == 2 * radius[ax] for ax in axes):
            reason[b] = "rim"
            continue
        cube = c.reshape(window)
        s = np.zeros(ndim)
        for ax in range(ndim):
            s[ax] = k[ax] - radius[ax]
            if ax not in axes:
                continue
            below, above = list(k), list(k)
            below[ax] -= 1
            above[ax] += 1
            cm, cp = cube[tuple(below)], cube[tuple(above)]
            second = cm - 2.0 * c0 + cp
            if np.isnan(cm) or np.isnan(cp) or not second < 0:
                reason[b] = "flat"
                break
            s[ax] += np.clip(0.5 * (cm - cp) / second, -0.5, 0.5)
        if reason[b] is None:
            shift[b], weight[b] = s, n * c0
    return {"shift": shift, "weight": weight, "reason": reason, "ncc": peak_ncc, "n": peak_n}


# ---- the solver ---------------------------------------------------------------------------------------------------------------------
def solve_fields(nodes, records, linear_parts, spacings, lambda_identity=0.05, lambda_smooth=0.1, reference_view=None, return_info=False):
    """The fields that minimise the objective of ``fit_fields``, from shifts.  ``nodes``: per view its cells per axis; ``records``:
    an iterable of ``(view_f, view_m, cell_f, cell_m, s_world, w)``; ``linear_parts`` / ``spacings``: per view the linear part ``L_v``
    of its affine and its pixel spacing.  Host only, float64: the unknowns are one world-unit vector ``u`` per cell, the axes
    decouple (one matrix, ``ndim`` right-hand sides), dense up to ``intensity.DENSE_SOLVE_MAX_UNKNOWNS`` cells and sparse above.
    Returns the list of float32 fields ``nodes_v + (ndim,)``, ``d = (L_v^-1 u) / spacing_v`` (and the info dict: ``"pairs"``
    {(i, j): {"used", "w", "rms_before", "rms_after"}}, ``w`` the pair's sum of weights, and ``"W"``)."""
    if not lambda_identity > 0:
        raise ValueError("lambda_identity must be positive: it fixes the gauge (the data term only sees differences of fields)")
    nodes = [tuple(int(c) for c in nv) for nv in nodes]
    ndim = len(nodes[0])
    sizes = [int(np.prod(nv)) for nv in nodes]
    first = np.concatenate([[0], np.cumsum(sizes)])
    n_cells = int(first[-1])
    recs = [(int(vf), int(vm), tuple(int(c) for c in cf), tuple(int(c) for c in cm), np.asarray(s, dtype=np.float64), float(w))
            for vf, vm, cf, cm, s, w in records]
    u = np.zeros((n_cells, ndim))
    info = {"pairs": {}, "W": 0.0}
    W = sum(r[5] for r in recs)
    if recs and W > 0:
        from scipy import sparse

        info["W"] = float(W)
        kf = np.array([first[vf] + np.ravel_multi_index(cf, nodes[vf]) for vf, _, cf, _, _, _ in recs], dtype=np.int64)
        km = np.array([first[vm] + np.ravel_multi_index(cm, nodes[vm]) for _, vm, _, cm, _, _ in recs], dtype=np.int64)
        w = np.array([r[5] for r in recs])
        s = np.array([r[4] for r in recs]).reshape(len(recs), ndim)
        w_id, w_sm = lambda_identity * W / n_cells, lambda_smooth * W / n_cells
        rows, cols, vals = [km, kf, km, kf], [km, kf, kf, km], [w, w, -w, -w]
        rhs = np.zeros((n_cells, ndim))
        np.add.at(rhs, km, w[:, None] * s)
        np.add.at(rhs, kf, -w[:, None] * s)
        diag = np.arange(n_cells)
        rows.append(diag), cols.append(diag), vals.append(np.full(n_cells, w_id))
        if w_sm > 0:
            for v, nv in enumerate(nodes):
                ids = first[v] + np.arange(sizes[v]).reshape(nv)
                for ax in range(ndim):
                    a = np.take(ids, np.arange(nv[ax] - 1), axis=ax).ravel()
                    b = np.take(ids, np.arange(1, nv[ax]), axis=ax).ravel()
                    rows.extend([a, b, a, b]), cols.extend([a, b, b, a])
                    vals.extend([np.full(len(a), w_sm)] * 2 + [np.full(len(a), -w_sm)] * 2)
        H = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n_cells, n_cells)).tocsc()
        free = np.ones(n_cells, dtype=bool)
        if reference_view is not None:
            free[first[reference_view]:first[reference_view + 1]] = False
        fi = np.nonzero(free)[0]
        Hff = H[fi][:, fi]                              # (the fixed cells are at 0: they add nothing to the right-hand side)
        if Hff.shape[0] <= intensity.DENSE_SOLVE_MAX_UNKNOWNS:
            u[fi] = np.linalg.solve(Hff.toarray(), rhs[fi])
        else:
            from scipy.sparse.linalg import splu

            u[fi] = splu(Hff.tocsc()).solve(rhs[fi])
        res = u[km] - u[kf] - s
        for (vf, vm, *_), wi, si, ri in zip(recs, w, s, res):
            p = info["pairs"].setdefault((min(vf, vm), max(vf, vm)), {"used": 0, "w": 0.0, "before": 0.0, "after": 0.0})
            p["used"] += 1
            p["w"] += wi
            p["before"] += wi * float(si @ si)
            p["after"] += wi * float(ri @ ri)
        for p in info["pairs"].values():
            p["rms_before"], p["rms_after"] = float(np.sqrt(p.pop("before") / p["w"])), float(np.sqrt(p.pop("after") / p["w"]))
    fields = []
    for v, nv in enumerate(nodes):
        uv = u[first[v]:first[v + 1]]
        d = (uv @ np.linalg.inv(np.asarray(linear_parts[v], dtype=np.float64)).T) / np.asarray(spacings[v], dtype=np.float64)
        fields.append(d.reshape(nv + (ndim,)).astype(np.float32))
    return (fields, info) if return_info else fields


# ---- public entry points -----------------------------------------------------------------------------------------------------------
def _per_axis(value, ndim, default3, default2, name):
    if value is None:
        value = default3 if ndim == 3 else default2
    out = (int(value),) * ndim if isinstance(value, (int, np.integer)) else tuple(int(v) for v in value)
    if len(out) != ndim:
        raise ValueError(f"{name}: an int, or one per axis")
    return out


def fit_fields(msims, transform_key, nodes=4, pairs=None, block=None, radius=None, step=1, channel_index=0, overlap_tolerance=0.0,
               lambda_identity=0.05, lambda_smooth=0.1, min_samples=64, min_ncc=0.3, reference_view=None, device=0, return_info=False):
    """Displacement fields that make the views of ``msims`` agree in their overlaps under ``transform_key``: a list of float32
    arrays of shape ``nodes_v + (ndim,)`` (pixels of the view; z, y, x), one per view, for ``apply_fields``.

    ``msims``, ``pairs``, ``step`` and ``channel_index`` follow ``intensity.fit_maps``: multiscale or spatial images, numpy- or
    ``DeviceArray``-backed; each undirected pair once, the lower index as the fixed view; the overlap sampled linearly on a grid of
    ``step`` fixed pixels.  ``nodes``: cells per axis (1 .. 16) -- an int, a tuple, or one tuple per view.  The overlap grid of a
    pair is tiled into blocks of ``block`` grid points per axis (default 12 in 3-D, 32 in 2-D); for every block mvs_block_match
    gives the moments of all integer shifts within ``radius`` (default 3 in 3-D, 6 in 2-D), ``shifts_from_moments`` the sub-pixel
    shift ``s`` of the NCC peak and its weight ``w = n * ncc``, or the reason the block is dropped (``min_samples``, ``min_ncc``).

    With ``s_world = L_F (step * spacing_F * s)``, ``L_F`` the linear part of the fixed view's affine, a kept block is a record
    between the cell of its centre in the fixed and in the moving tile (``plan_blocks``), and ``W = sum w``.  The fields minimise, in
    float64, over one world-unit vector ``u`` per cell,

      sum over records of  w |u_M,cell_m - u_F,cell_f - s_world|^2                                   (data)
      + lambda_identity * W / n_cells_total * sum over cells |u|^2                                    (identity)
      + lambda_smooth * W / n_cells_total * sum over adjacent cells of a view |u - u'|^2              (smoothness)

    and view ``v`` gets ``d = (L_v^-1 u) / spacing_v``.  ``lambda_identity`` must be positive (it fixes the gauge);
    ``reference_view`` keeps that view at 0.  A view without a kept block gets what the regularisers give it: zeros.

    ``return_info=True``: also a dict with ``"pairs"``: {(i, j): {"used", "w", "dropped": {reason: count}, "rms_before", "rms_after"}}
    -- the weighted RMS of ``|s_world|`` and of the residual ``|u_M - u_F - s_world|`` at the solution (NaN without a kept block)
    --, ``"W"``, and ``"blocks"``: {(i, j): the dict of ``shifts_from_moments`` plus ``"blocks"``, the rows of ``plan_blocks``}."""
    if not lambda_identity > 0:
        raise ValueError("lambda_identity must be positive: it fixes the gauge (the data term only sees differences of fields)")
    sims = [intensity._fit_sim(m, channel_index) for m in msims]
    ndim = len(si_utils.get_spatial_dims_from_sim(sims[0]))
    per_view = intensity._cells_per_view(nodes, len(sims), ndim)
    block = _per_axis(block, ndim, 12, 32, "block")
    radius = _per_axis(radius, ndim, 3, 6, "radius")
    if any(r < 0 or r > _lib.MVS_BLOCKMATCH_MAX_RADIUS for r in radius):
        raise ValueError(f"radius per axis must be 0..{_lib.MVS_BLOCKMATCH_MAX_RADIUS}")
    if np.prod(block) + np.prod([b + 2 * r for b, r in zip(block, radius)]) > _lib.MVS_BLOCKMATCH_MAX_FLOATS:
        raise ValueError(f"block and radius: prod block + prod (block + 2 radius) must not exceed {_lib.MVS_BLOCKMATCH_MAX_FLOATS}")
    if pairs is None:
        pairs = intensity.view_pairs(sims, transform_key, overlap_tolerance)
    pairs = sorted({(min(int(i), int(j)), max(int(i), int(j))) for i, j in pairs})
    linear = [np.asarray(metrics._affine(s, transform_key), dtype=np.float64)[:ndim, :ndim] for s in sims]
    spacings = [si_utils.get_spacing_from_sim(s, asarray=True) for s in sims]
    records, dropped, matched = [], {}, {}
    for i, j in pairs:
        geo = intensity.pair_geometry(sims[i], sims[j], transform_key, step, overlap_tolerance)
        if geo is None:
            continue
        blocks = plan_blocks(geo["grid_shape"], block, geo["fixed_affine"], geo["moving_affine"], sims[i].shape, sims[j].shape, per_view[i], per_view[j])
        moments = _nonrigid_ops.block_match(sims[i].data, sims[j].data, geo["fixed_affine"], geo["moving_affine"], blocks, radius,
                                            geo["halfspaces"], device)
        found = shifts_from_moments(moments, radius, min_samples, min_ncc)
        dropped[(i, j)] = {r: sum(1 for x in found["reason"] if x == r) for r in DROP_REASONS}
        matched[(i, j)] = dict(found, blocks=blocks)
        for b, s, w, why in zip(blocks, found["shift"], found["weight"], found["reason"]):
            if why is None:
                records.append((i, j, tuple(b[2]), tuple(b[3]), linear[i] @ (float(step) * spacings[i] * s), w))
    fields, info = solve_fields(per_view, records, linear, spacings, lambda_identity, lambda_smooth, reference_view, True)
    for pair, d in dropped.items():
        info["pairs"].setdefault(pair, {"used": 0, "w": 0.0, "rms_before": float("nan"), "rms_after": float("nan")})["dropped"] = d
    info["blocks"] = matched
    return (fields, info) if return_info else fields


def apply_fields(msims, fields, out_dtype=None, device=0):
    """``I'(p) = I(clamp(p + d(p), 0, n - 1))`` for every view (mvs_field_warp): images of the kind given -- multiscale or spatial,
    host or resident -- with all attributes, transforms, coordinates and point sets carried over as ``intensity.apply_maps`` does.

    ``fields``: per view one array ``nodes + (ndim,)`` (``fit_fields``), applied to all channels and time points.  ``out_dtype``:
    the view's dtype (default; integer results are rounded half to even and saturated) or float32.  Never in place: the kernel
    gathers.  Of a multiscale image only scale0 goes through the kernel; the further levels are rebuilt as by ``apply_maps``."""
    if len(fields) != len(msims):
        raise ValueError("one field per view")
    return intensity._apply_views(msims, fields, out_dtype, False, device, _nonrigid_ops.warp_field, "apply_fields")
