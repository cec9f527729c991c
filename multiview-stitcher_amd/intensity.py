"""Tile intensity harmonisation on the HIP backend: remove brightness steps between tiles and views before fusion.

Bleaching, the light-sheet side, detector offsets and per-tile exposure leave steps between tiles that blending only smears over
the overlap.  ``fit_maps`` estimates, per view, a coarse grid of gains and offsets from the image content of the overlaps (the
"intensity adjustment in overlaps" of BigStitcher; the reference has no counterpart), ``apply_maps`` corrects whole tiles with
them before ``fusion.fuse``.

Model: view ``v`` has ``cells_v = (gz, gy, gx)`` cells with a gain ``a`` and an offset ``b`` each.  Along an axis of ``n`` pixels
with ``g`` cells the coordinate ``c`` belongs to cell ``clamp(floor((c + 0.5) * g / n), 0, g - 1)`` and the centre of cell ``k`` is
at ``(k + 0.5) * n / g - 0.5`` (``_intensity_ops.cell_index`` / ``cell_centres``; the kernels use the same rule).  The fit treats
``a, b`` as constant per cell; the correction ``I' = a(p) I + b(p)`` interpolates them multilinearly between the cell centres.

The voxel work runs in two kernels (csrc/mvs_intensity.hip): mvs_intensity_pair_moments reduces the overlap of a pair to six
moments per pair of cells, mvs_intensity_apply corrects a tile.  The planner and the solver below are host algebra in float64.

``estimate_shading`` / ``apply_shading`` remove what the overlaps cannot show: the shading every tile shares (vignetting, uneven
illumination).  The per-pixel order statistics of the stack of all tiles come from mvs_stack_quantiles, the correction runs in
mvs_plane_apply (csrc/mvs_shading.hip); the smoothing and normalisation between the two are host algebra in float64."""

from __future__ import annotations

import numpy as np

from . import _intensity_ops, _shading_ops, metrics, msi_utils, mv_graph
from . import spatial_image_utils as si_utils
from ._intensity_ops import axis_table, cell_centres, cell_index  # noqa: F401  (part of this module's interface)
from .transformation import get_pixel_affine

DENSE_SOLVE_MAX_UNKNOWNS = 2000


# ---- records of one pair -----------------------------------------------------------------------------------------------------------
def _is_diagonal(matrix):
    m = np.asarray(matrix, dtype=np.float64)
    return not np.any(m - np.diag(np.diag(m))) and np.all(np.diag(m) != 0)


def _cell_boxes(affine, grid_shape, shape, cells):
    """Per cell of one tile (C order over ``cells``) the half-open box ``[lo, hi)`` of grid indices that can hold its samples.
    Axis-aligned map: exact, from the cell rule evaluated on every index of each axis with the kernel's own arithmetic.  General
    affine: the bounding box of the cell's preimage, grown by one index, clipped to the grid."""
    matrix, offset = np.asarray(affine[0], dtype=np.float64), np.asarray(affine[1], dtype=np.float64)
    ndim = len(grid_shape)
    multi = np.array(list(np.ndindex(*cells)), dtype=np.int64).reshape(-1, ndim)
    lo = np.zeros((len(multi), ndim), dtype=np.int64)
    hi = np.zeros((len(multi), ndim), dtype=np.int64)
    if _is_diagonal(matrix):
        for ax in range(ndim):
            c = np.arange(grid_shape[ax], dtype=np.float64) * matrix[ax, ax] + offset[ax]
            inb = (c >= 0) & (c <= shape[ax] - 1)
            k = cell_index(c, cells[ax], shape[ax])
            for cell in range(cells[ax]):
                idx = np.nonzero(inb & (k == cell))[0]
                sel = multi[:, ax] == cell
                if len(idx):            # (monotone in the index: a run)
                    lo[sel, ax], hi[sel, ax] = idx[0], idx[-1] + 1
        return multi, lo, hi
    inv = np.linalg.inv(matrix)
    corners = np.array(list(np.ndindex(*([2] * ndim))), dtype=np.float64)
    n = np.asarray(shape, dtype=np.float64)
    g = np.asarray(cells, dtype=np.float64)
    for i, cell in enumerate(multi):
        plo = np.maximum(cell * n / g - 0.5, 0.0)                 # the cell's pixel box, inside the tile's sampling bounds
        phi = np.minimum((cell + 1) * n / g - 0.5, n - 1.0)
        if np.any(plo > phi):
            continue
        pts = (plo + corners * (phi - plo) - offset) @ inv.T
        lo[i] = np.clip(np.floor(pts.min(axis=0)).astype(np.int64) - 1, 0, grid_shape)
        hi[i] = np.clip(np.ceil(pts.max(axis=0)).astype(np.int64) + 2, 0, grid_shape)
    return multi, lo, hi


def plan_records(fixed_affine, moving_affine, grid_shape, shape_f, shape_m, cells_f, cells_m):
    """The records of one pair for mvs_intensity_pair_moments: an int64 array ``(R, 4, ndim)`` with the rows ``lo, n, cell_f,
    cell_m``.  Host only.

    ``fixed_affine`` / ``moving_affine = (matrix, offset)`` map an index of the grid of ``grid_shape`` to a pixel of the tile of
    ``shape_f`` / ``shape_m``.  For every cell of the fixed tile that meets the grid and every cell of the moving tile whose
    preimage can meet it, the record's box is the intersection of the two cells' boxes in grid index: exact for axis-aligned maps
    (the boxes then tile the overlap without overlapping each other), else the bounding boxes of the preimages grown by one index.
    Empty boxes are dropped.  The kernel tests every voxel against the cell rule, so boxes only need to be conservative."""
    grid_shape = tuple(int(s) for s in grid_shape)
    ndim = len(grid_shape)
    cells_f, cells_m = tuple(int(c) for c in cells_f), tuple(int(c) for c in cells_m)
    mf, lof, hif = _cell_boxes(fixed_affine, grid_shape, shape_f, cells_f)
    mm, lom, him = _cell_boxes(moving_affine, grid_shape, shape_m, cells_m)
    lo = np.maximum(lof[:, None, :], lom[None, :, :])
    hi = np.minimum(hif[:, None, :], him[None, :, :])
    keep_f, keep_m = np.nonzero(np.all(hi > lo, axis=2))
    out = np.zeros((len(keep_f), 4, ndim), dtype=np.int64)
    out[:, 0] = lo[keep_f, keep_m]
    out[:, 1] = hi[keep_f, keep_m] - lo[keep_f, keep_m]
    out[:, 2] = mf[keep_f]
    out[:, 3] = mm[keep_m]
    return out


# ---- the solver ---------------------------------------------------------------------------------------------------------------------
def _raw_sums(m):
    """(n, Sf, Sm, Sff, Smm, Sfm) of one row of moments."""
    n, mf, mm, m2f, m2m, cfm = (float(v) for v in m)
    return n, n * mf, n * mm, m2f + n * mf * mf, m2m + n * mm * mm, cfm + n * mf * mm


def _pair_form(m, s):
    """G with ``sum (a_F f + b_F - a_M m - b_M)^2 / s^2 = u^T G u`` for ``u = (a_F, b_F / s, a_M, b_M / s)``."""
    n, sf, sm, sff, smm, sfm = _raw_sums(m)
    sf, sm, sff, smm, sfm = sf / s, sm / s, sff / (s * s), smm / (s * s), sfm / (s * s)
    return np.array([[sff, sf, -sfm, -sf], [sf, n, -sm, -n], [-sfm, -sm, smm, sm], [-sf, -n, sm, n]])


def solve_maps(cells, records, lambda_identity=0.05, lambda_smooth=0.1, min_samples=64, reference_view=None, normalize=True,
               return_info=False):
    """The maps that minimise the objective of ``fit_maps``, from moments.  ``cells``: per view its cells per axis; ``records``: an
    iterable of ``(view_f, view_m, cell_f, cell_m, moments)`` with ``moments`` a row of ``cell_pair_moments``.  Host only, float64.
    Returns the list of float32 maps ``cells_v + (2,)`` (and the info dict of ``fit_maps``)."""
    if not lambda_identity > 0:
        raise ValueError("lambda_identity must be positive: the data term alone is minimised by a = 0")
    cells = [tuple(int(c) for c in cv) for cv in cells]
    sizes = [int(np.prod(cv)) for cv in cells]
    first = np.concatenate([[0], np.cumsum(sizes)])
    n_cells = int(first[-1])
    used, skipped = [], []
    for vf, vm, cf, cm, m in records:
        m = np.asarray(m, dtype=np.float64)
        (used if m[0] >= min_samples and m[0] > 0 else skipped).append((int(vf), int(vm), tuple(int(c) for c in cf), tuple(int(c) for c in cm), m))
    maps64 = [np.tile(np.array([1.0, 0.0]), cv + (1,)) for cv in cells]
    info = {"pairs": {}, "skipped": [(vf, vm, cf, cm, float(m[0])) for vf, vm, cf, cm, m in skipped], "s": 1.0, "N": 0.0}
    if used:
        N = sum(m[0] for *_, m in used)
        sq = sum(_raw_sums(m)[3] + _raw_sums(m)[4] for *_, m in used)
        s = float(np.sqrt(sq / (2.0 * N)))
        if not s > 0:
            s = 1.0
        info.update(s=s, N=float(N))
        # unknown 2 * cell: the gain, 2 * cell + 1: the offset in units of s
        rows, cols, vals = [], [], []
        w_id = lambda_identity * N / n_cells
        w_sm = lambda_smooth * N / n_cells
        rhs = np.zeros(2 * n_cells)
        forms = []
        for vf, vm, cf, cm, m in used:
            G = _pair_form(m, s)
            kf = int(first[vf] + np.ravel_multi_index(cf, cells[vf]))
            km = int(first[vm] + np.ravel_multi_index(cm, cells[vm]))
            idx = np.array([2 * kf, 2 * kf + 1, 2 * km, 2 * km + 1])
            forms.append(((min(vf, vm), max(vf, vm)), idx, G, m[0]))
            rows.append(np.repeat(idx, 4)), cols.append(np.tile(idx, 4)), vals.append(G.ravel())
        diag = np.arange(2 * n_cells)
        rows.append(diag), cols.append(diag), vals.append(np.full(2 * n_cells, w_id))
        rhs[0::2] = w_id
        if w_sm > 0:
            for v, cv in enumerate(cells):
                ids = first[v] + np.arange(sizes[v]).reshape(cv)
                for ax in range(len(cv)):
                    a = np.take(ids, np.arange(cv[ax] - 1), axis=ax).ravel()
                    b = np.take(ids, np.arange(1, cv[ax]), axis=ax).ravel()
                    for comp in (0, 1):
                        i, j = 2 * a + comp, 2 * b + comp
                        rows.extend([i, j, i, j]), cols.extend([i, j, j, i])
                        vals.extend([np.full(len(i), w_sm)] * 2 + [np.full(len(i), -w_sm)] * 2)
        from scipy import sparse

        H = sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * n_cells, 2 * n_cells)).tocsc()
        u = np.zeros(2 * n_cells)
        u[0::2] = 1.0
        free = np.ones(2 * n_cells, dtype=bool)
        if reference_view is not None:
            free[2 * first[reference_view]:2 * first[reference_view + 1]] = False
        fi, ci = np.nonzero(free)[0], np.nonzero(~free)[0]
        b = rhs[fi] - H[fi][:, ci] @ u[ci]
        Hff = H[fi][:, fi]
        if Hff.shape[0] <= DENSE_SOLVE_MAX_UNKNOWNS:
            u[free] = np.linalg.solve(Hff.toarray(), b)
        else:
            from scipy.sparse.linalg import splu

            u[free] = splu(Hff.tocsc()).solve(b)
        ident = np.zeros(2 * n_cells)
        ident[0::2] = 1.0
        for pair, idx, G, n in forms:
            p = info["pairs"].setdefault(pair, {"n": 0.0, "data_before": 0.0, "data_after": 0.0})
            p["n"] += float(n)
            p["data_before"] += float(ident[idx] @ G @ ident[idx])
            p["data_after"] += float(u[idx] @ G @ u[idx])
        for v, cv in enumerate(cells):
            part = u[2 * first[v]:2 * first[v + 1]].reshape(cv + (2,)).copy()
            part[..., 1] *= s
            maps64[v] = part
    if normalize and reference_view is None:
        # one global affine I'' = alpha I' + beta for all views: the mean gain over cells becomes 1, the mean offset 0
        alpha = 1.0 / np.mean(np.concatenate([m[..., 0].ravel() for m in maps64]))
        beta = -alpha * np.mean(np.concatenate([m[..., 1].ravel() for m in maps64]))
        for m in maps64:
            m[..., 0] *= alpha
            m[..., 1] = alpha * m[..., 1] + beta
    maps = [m.astype(np.float32) for m in maps64]
    return (maps, info) if return_info else maps


# ---- public entry points -----------------------------------------------------------------------------------------------------------
def _as_sim(image):
    return msi_utils.get_sim_from_msim(image, scale="scale0") if msi_utils.is_msim(image) else image


def _fit_sim(image, channel_index):
    """The spatial image a view is fitted on: channel ``channel_index``, the first time point."""
    sim = _as_sim(image)
    sel = {d: (channel_index if d == "c" else 0) for d in sim.dims if d in ("c", "t")}
    return sim.isel(sel) if sel else sim


def _cells_per_view(cells, n_views, ndim):
    if isinstance(cells, (int, np.integer)):
        per = [(int(cells),) * ndim] * n_views
    elif len(cells) and isinstance(cells[0], (int, np.integer)):
        per = [tuple(int(c) for c in cells)] * n_views
    else:
        per = [tuple(int(c) for c in cv) for cv in cells]
    if len(per) != n_views or any(len(cv) != ndim for cv in per):
        raise ValueError("cells: an int, one tuple per axis, or one such tuple per view")
    if any(c < 1 or c > _intensity_ops._lib.MVS_INTENSITY_MAX_CELLS for cv in per for c in cv):
        raise ValueError(f"cells per axis must be 1..{_intensity_ops._lib.MVS_INTENSITY_MAX_CELLS}")
    return per


def pair_geometry(sim_fixed, sim_moving, transform_key, step=1, overlap_tolerance=0.0):
    """The overlap grid of one pair under ``transform_key`` as the kernels take it: ``None`` without an overlap, else a dict with
    ``grid_shape``, ``fixed_affine`` and ``moving_affine`` (grid index -> pixel) and ``halfspaces`` (grid index coordinates).  The
    grid is that of ``metrics.tile_pair_image_metrics`` with a spacing of ``step`` fixed pixels and the same halfspace expansion."""
    tol = float(overlap_tolerance) if overlap_tolerance else None
    geo = metrics._overlap_geometry(sim_fixed, sim_moving, transform_key, tol)
    if geo["comparison_bbox"] is None:
        return None
    ndim = len(si_utils.get_spatial_dims_from_sim(sim_fixed))
    fixed_spacing = si_utils.get_spacing_from_sim(sim_fixed, asarray=True)
    spacing = fixed_spacing * float(step)
    origin, shape = metrics.comparison_grid(geo["comparison_bbox"], spacing)
    equations = np.array(geo["halfspaces"], dtype=np.float64)
    equations[:, -1] -= metrics.HALFSPACE_EXPANSION * np.min(fixed_spacing)
    p_moving = np.linalg.inv(metrics._affine(sim_moving, transform_key)) @ metrics._affine(sim_fixed, transform_key)
    return {
        "grid_shape": shape,
        "halfspaces": metrics.halfspaces_to_grid_index(equations, origin, spacing),
        "fixed_affine": get_pixel_affine(np.eye(ndim + 1), si_utils.get_origin_from_sim(sim_fixed, asarray=True), fixed_spacing, origin, spacing),
        "moving_affine": get_pixel_affine(p_moving, si_utils.get_origin_from_sim(sim_moving, asarray=True),
                                          si_utils.get_spacing_from_sim(sim_moving, asarray=True), origin, spacing),
    }


def view_pairs(sims, transform_key, overlap_tolerance=0.0):
    """The overlapping pairs of ``sims`` (edges of ``mv_graph.build_view_adjacency_graph``), each once as (lower, higher) index."""
    views = [dict(si_utils.get_stack_properties_from_sim(s), transform=metrics._affine(s, transform_key)) for s in sims]
    g = mv_graph.build_view_adjacency_graph(views, overlap_tolerance=float(overlap_tolerance) if overlap_tolerance else None)
    return sorted({(min(i, j), max(i, j)) for i, j in g.edges()})


def fit_maps(msims, transform_key, cells=1, pairs=None, step=1, channel_index=0, overlap_tolerance=0.0, lambda_identity=0.05,
             lambda_smooth=0.1, min_samples=64, reference_view=None, normalize=True, device=0, return_info=False):
    """Gain / offset maps that make the views of ``msims`` agree in their overlaps under ``transform_key``: a list of float32
    arrays of shape ``cells_v + (2,)`` (``[..., 0]`` gain, ``[..., 1]`` offset), one per view, for ``apply_maps``.

    ``msims``: multiscale or spatial images, numpy- or ``DeviceArray``-backed (resident tiles are read in place); views with
    ``c`` / ``t`` dims are fitted on channel ``channel_index`` of the first time point.  ``cells``: cells per axis -- an int, a
    tuple, or one tuple per view.  ``pairs``: the (i, j) to use (default: the overlapping pairs of the view adjacency graph); each
    undirected pair is used once, the lower index as the fixed view.  The overlap is sampled linearly on a grid of ``step`` fixed
    pixels, as ``metrics.tile_pair_image_metrics`` does, and reduced on the device to six moments per pair of cells
    (mvs_intensity_pair_moments); records of fewer than ``min_samples`` pairs are ignored.

    With ``N`` the number of counted sample pairs and ``s`` the RMS of their 2 N samples, the maps minimise, in float64,

      sum over records of  sum (a_F f + b_F - a_M m - b_M)^2 / s^2                                  (data)
      + lambda_identity * N / n_cells_total * sum over cells [(a - 1)^2 + (b / s)^2]                 (identity)
      + lambda_smooth * N / n_cells_total * sum over adjacent cells of a view [(a - a')^2 + ((b - b') / s)^2]   (smoothness)

    ``lambda_identity`` must be positive (the data term alone is minimised by ``a = 0``).  ``reference_view`` keeps that view at
    ``a = 1, b = 0``.  ``normalize`` rescales all maps by one global affine so that the mean gain over cells is 1 and the mean
    offset 0 (skipped with a ``reference_view``).  A view without a usable record keeps the identity map.

    ``return_info=True``: also a dict with ``"pairs"`` ({(i, j): {"n", "data_before", "data_after"}}, the data term at the
    identity and at the solution before normalisation), ``"skipped"`` (the ignored records as (i, j, cell_f, cell_m, n)), ``"s"``
    and ``"N"``."""
    if not lambda_identity > 0:
        raise ValueError("lambda_identity must be positive: the data term alone is minimised by a = 0")
    sims = [_fit_sim(m, channel_index) for m in msims]
    ndim = len(si_utils.get_spatial_dims_from_sim(sims[0]))
    per_view = _cells_per_view(cells, len(sims), ndim)
    if pairs is None:
        pairs = view_pairs(sims, transform_key, overlap_tolerance)
    pairs = sorted({(min(int(i), int(j)), max(int(i), int(j))) for i, j in pairs})
    records = []
    for i, j in pairs:
        geo = pair_geometry(sims[i], sims[j], transform_key, step, overlap_tolerance)
        if geo is None:
            continue
        recs = plan_records(geo["fixed_affine"], geo["moving_affine"], geo["grid_shape"], sims[i].shape, sims[j].shape, per_view[i], per_view[j])
        if not len(recs):
            continue
        moments = _intensity_ops.cell_pair_moments(sims[i].data, sims[j].data, geo["fixed_affine"], geo["moving_affine"], per_view[i],
                                                   per_view[j], recs, geo["halfspaces"], device)
        records.extend((i, j, tuple(r[2]), tuple(r[3]), m) for r, m in zip(recs, moments))
    return solve_maps(per_view, records, lambda_identity, lambda_smooth, min_samples, reference_view, normalize, return_info)


def _apply_sim(sim, vmap, out_dtype, inplace, device, apply_one=_intensity_ops.apply_map, who="apply_maps"):
    """One spatial image through ``apply_one(data, coeff, out=, out_dtype=, device=)``, leading c / t dims looped; ``vmap``: the
    coefficients, or a dict of them per channel coordinate."""
    from .device import DeviceArray, is_device_array

    lead = [d for d in sim.dims if d in ("c", "t")]
    if list(sim.dims[:len(lead)]) != lead:
        raise ValueError(f"{who} needs the c / t dims in front of the spatial ones")
    data = sim.data
    on_dev = is_device_array(data)
    dtype = np.dtype(data.dtype) if out_dtype is None else np.dtype(out_dtype)
    if inplace:
        if dtype != np.dtype(data.dtype):
            raise ValueError("inplace=True keeps the dtype")
        out = data
    else:
        out = DeviceArray.empty(data.shape, dtype, device) if on_dev else np.empty(data.shape, dtype=dtype)
    for idx in np.ndindex(*data.shape[:len(lead)]):
        if isinstance(vmap, dict):
            coeff = vmap[sim.coords["c"][idx[lead.index("c")]].item() if "c" in lead else next(iter(vmap))]
        else:
            coeff = vmap
        apply_one(data[idx] if idx else data, coeff, out=out[idx] if idx else out, out_dtype=dtype, device=device)
    return sim if inplace else sim.copy(data=out)


def _apply_views(msims, per_view, out_dtype, inplace, device, apply_one=_intensity_ops.apply_map, who="apply_maps"):
    """Every view through ``_apply_sim`` with its own coefficients; multiscale images are rebuilt around the corrected scale0."""
    from .device import is_device_array

    out = []
    for image, vmap in zip(msims, per_view):
        sim = _apply_sim(_as_sim(image), vmap, out_dtype, inplace, device, apply_one, who)
        if not msi_utils.is_msim(image):
            out.append(sim)
            continue
        sim.attrs["transforms"] = {k: np.array(v, dtype=np.float64, copy=True) for k, v in image.transforms.items()}
        factors = []
        if not is_device_array(sim.data):
            keys = msi_utils.get_sorted_scale_keys(image)
            sdims = si_utils.get_spatial_dims_from_sim(sim)
            for a, b in zip(keys, keys[1:]):
                sa, sb = si_utils.get_spacing_from_sim(image[a]), si_utils.get_spacing_from_sim(image[b])
                factors.append({d: int(round(sb[d] / sa[d])) for d in sdims})
        res = msi_utils.get_msim_from_sim(sim, scale_factors=factors)
        res.point_sets = dict(getattr(image, "point_sets", {}))
        out.append(res)
    return out


def apply_maps(msims, maps, out_dtype=None, inplace=False, device=0):
    """``I' = a(p) I + b(p)`` for every view (mvs_intensity_apply): images of the kind given -- multiscale or spatial, host or
    resident -- with all attributes, transforms and coordinates carried over.

    ``maps``: per view one array ``cells + (2,)`` (``fit_maps``), applied to all channels and time points, or a dict of such
    arrays per channel coordinate.  ``out_dtype``: the view's dtype (default; integer results are rounded half to even and
    saturated) or float32.  ``inplace=True`` overwrites the views' (contiguous) arrays.  Leading ``c`` / ``t`` dims are looped.

    Of a multiscale image only scale0 goes through the kernel.  The further levels of a host-backed image are rebuilt from the
    corrected scale0 by ``msi_utils.get_msim_from_sim`` with the factors of the given pyramid; a resident image keeps scale0
    only (the pyramid helper averages on the host)."""
    if len(maps) != len(msims):
        raise ValueError("one map per view")
    return _apply_views(msims, maps, out_dtype, inplace, device)


# ---- shading (flat-field) correction ---------------------------------------------------------------------------------------------
# fit_maps sees only the overlaps, so it cannot remove what every tile shares: the vignetting and uneven illumination of the one
# objective and camera, which leave a lattice across a fused mosaic.  The retrospective estimate of that profile is a per-pixel
# order statistic over the stack of all tiles and planes (mvs_stack_quantiles), smoothed and normalised to mean 1 on the host;
# the correction I' = (I - D) / F + mean(D) is one gain and one offset per pixel (mvs_plane_apply).  The reference has no
# counterpart; BigStitcher's flat-field correction, MIST and BaSiC are the model (BaSiC's low-rank fit is out of scope).
# The median of a pixel sees the background only where the sample is sparse: ``quantile`` is the knob.
SHADING_FIT_ROWS = 256            # rows of the design matrix of the polynomial fit that are built at a time


def _unit_coordinates(n):
    return np.zeros(1) if n == 1 else np.linspace(-1.0, 1.0, n)


def _legendre_smooth(plane, valid, degree):
    """Least squares fit of ``plane`` on ``valid`` by the products ``P_i(y) P_j(x)``, ``i + j <= degree``, of Legendre polynomials
    in coordinates scaled to [-1, 1], evaluated on all pixels."""
    from numpy.polynomial import legendre

    h, w = plane.shape
    vy, vx = legendre.legvander(_unit_coordinates(h), degree), legendre.legvander(_unit_coordinates(w), degree)
    terms = [(i, j) for i in range(degree + 1) for j in range(degree + 1 - i)]
    if int(valid.sum()) < len(terms):
        raise ValueError(f"shading: {int(valid.sum())} usable pixels cannot carry a polynomial of {len(terms)} terms")
    ti, tj = np.array([t[0] for t in terms]), np.array([t[1] for t in terms])
    ata, atb = np.zeros((len(terms), len(terms))), np.zeros(len(terms))
    for y0 in range(0, h, SHADING_FIT_ROWS):
        rows = slice(y0, min(y0 + SHADING_FIT_ROWS, h))
        a = (vy[rows][:, None, ti] * vx[None, :, tj])[valid[rows]]
        ata += a.T @ a
        atb += a.T @ plane[rows][valid[rows]]
    coef = np.linalg.lstsq(ata, atb, rcond=None)[0]
    cmat = np.zeros((degree + 1, degree + 1))
    cmat[ti, tj] = coef
    return vy @ cmat @ vx.T


def _smooth_plane(plane, valid, degree, sigma):
    """``plane`` (float64) smoothed over its ``valid`` pixels and filled in on the others: polynomial (``degree``), NaN-aware
    normalised Gaussian (``sigma``, mode="nearest"), or as it is with the mean of the valid pixels elsewhere."""
    if not valid.any():
        raise ValueError("shading: no pixel has enough samples")
    if degree is not None and sigma is not None:
        raise ValueError("shading: give degree or sigma, not both")
    if degree is not None:
        return _legendre_smooth(np.where(valid, plane, 0.0), valid, int(degree))
    if sigma is not None:
        from scipy import ndimage

        num = ndimage.gaussian_filter(np.where(valid, plane, 0.0), sigma, mode="nearest")
        den = ndimage.gaussian_filter(valid.astype(np.float64), sigma, mode="nearest")
        ok = den > 1e-12
        res = np.where(ok, num / np.where(ok, den, 1.0), 0.0)
        return np.where(ok, res, res[ok].mean())
    return np.where(valid, plane, plane[valid].mean())


def shading_from_planes(planes, counts, darkfield=None, degree=4, sigma=None, min_samples=8, min_flat=0.1):
    """The shading model from the order statistics of ``_shading_ops.stack_quantiles``.  Host only, float64.

    ``R = planes[-1] - D``.  ``darkfield``: ``None`` (D = 0), a scalar or an ``(H, W)`` array the caller measured, or
    ``"quantile"``: the smoothed ``planes[0]`` (``estimate_shading(dark_quantile=...)``).  Pixels with ``counts < min_samples`` or a
    non-finite R are left out of the fit.  Smoothing: ``degree`` -- least squares on the products of Legendre polynomials of total
    degree <= ``degree`` in coordinates scaled to [-1, 1] (the default: a Gaussian biases a paraboloid by more than 10 % at the tile
    border); ``sigma`` (with ``degree=None``) -- a NaN-aware normalised Gaussian, mode="nearest"; neither -- the raw plane.  Then
    ``F /= mean(F)`` and ``F = max(F, min_flat)``.

    Returns ``{"flatfield": F, "darkfield": D, "offset": mean(D)}``: float32 ``(H, W)`` arrays and a float."""
    planes = np.asarray(planes, dtype=np.float64)
    counts = np.asarray(counts)
    if planes.ndim != 3 or counts.shape != planes.shape[1:]:
        raise ValueError("shading_from_planes needs planes (n_q, H, W) and counts (H, W)")
    enough = counts >= int(min_samples)
    if isinstance(darkfield, str):
        if darkfield != "quantile" or len(planes) < 2:
            raise ValueError('darkfield="quantile" needs two planes: the dark and the bright quantile')
        dark = _smooth_plane(planes[0], enough & np.isfinite(planes[0]), degree, sigma)
    elif darkfield is None:
        dark = np.zeros(planes.shape[1:])
    else:
        dark = np.broadcast_to(np.asarray(darkfield, dtype=np.float64), planes.shape[1:]).copy()
    with np.errstate(invalid="ignore"):
        raw = planes[-1] - dark
    flat = _smooth_plane(raw, enough & np.isfinite(raw), degree, sigma)
    flat = flat / flat.mean()
    flat = np.maximum(flat, float(min_flat))
    return {"flatfield": flat.astype(np.float32), "darkfield": dark.astype(np.float32), "offset": float(dark.mean())}


def shading_coefficients(shading):
    """The ``(H, W, 2)`` float32 gain / offset plane of a shading model for ``_shading_ops.apply_plane``: ``a = 1 / F``,
    ``b = offset - D / F``, derived in float64, so that ``I' = (I - D) / F + offset``."""
    flat = np.asarray(shading["flatfield"], dtype=np.float64)
    dark = np.broadcast_to(np.asarray(shading["darkfield"], dtype=np.float64), flat.shape)
    return np.stack([1.0 / flat, float(shading["offset"]) - dark / flat], axis=-1).astype(np.float32)


def _shading_tiles(msims, channel_index, plane_step):
    """The tiles of the stack: channel ``channel_index`` of every view and time point, every ``plane_step``-th plane by stride."""
    tiles = []
    for image in msims:
        sim = _as_sim(image)
        lead = [d for d in sim.dims if d in ("c", "t")]
        if list(sim.dims[:len(lead)]) != lead:
            raise ValueError("estimate_shading needs the c / t dims in front of the spatial ones")
        data = sim.data
        for idx in np.ndindex(*[1 if d == "c" else n for d, n in zip(lead, data.shape)]):
            idx = tuple(channel_index if d == "c" else i for d, i in zip(lead, idx))
            tiles.append(_shading_ops.every_kth_plane(data[idx] if idx else data, plane_step))
    return tiles


def estimate_shading(msims, channel_index=0, quantile=0.5, dark_quantile=None, plane_step=1, darkfield=None, degree=4, sigma=None,
                     min_samples=8, min_flat=0.1, device=0, return_info=False):
    """The shading all tiles of an acquisition share, for ``apply_shading``: ``{"flatfield", "darkfield", "offset"}``.

    ``msims``: multiscale or spatial images of one tile shape and dtype, numpy- or ``DeviceArray``-backed (resident tiles are read
    in place).  Channel ``channel_index`` of every view and time point and every ``plane_step``-th plane (by stride, no copy) form
    the stack; per pixel of the tile the sample of quantile ``quantile`` -- and of ``dark_quantile``, when given, as the dark field
    -- is selected on the device (mvs_stack_quantiles: exact, numpy's ``method="lower"``, NaNs left out) and handed to
    ``shading_from_planes`` with ``darkfield``, ``degree``, ``sigma``, ``min_samples`` and ``min_flat``.

    The estimate assumes that over the stack every pixel sees the same distribution of content: many tiles, and a ``quantile`` that
    lands on comparable structure everywhere (the median sees the background only where the sample is sparse).

    ``return_info=True``: also ``{"planes", "counts", "q"}``, the raw order statistics."""
    tiles = _shading_tiles(msims, channel_index, plane_step)
    q = [float(quantile)] if dark_quantile is None else [float(dark_quantile), float(quantile)]
    planes, counts = _shading_ops.stack_quantiles(tiles, q, device)
    shading = shading_from_planes(planes, counts, "quantile" if dark_quantile is not None else darkfield, degree, sigma, min_samples, min_flat)
    return (shading, {"planes": planes, "counts": counts, "q": q}) if return_info else shading


def apply_shading(msims, shading, out_dtype=None, inplace=False, device=0):
    """``I' = (I - D) / F + mean(D)`` for every view (mvs_plane_apply), with the conventions of ``apply_maps``: images of the kind
    given -- multiscale or spatial, host or resident -- leading ``c`` / ``t`` dims looped, ``out_dtype`` the view's dtype (rounded
    half to even and saturated) or float32, ``inplace=True`` overwriting contiguous arrays, the pyramid of a host-backed multiscale
    image rebuilt from the corrected scale0.

    ``shading``: one model (``estimate_shading``) for all channels, or a dict of models per channel coordinate.  The coefficient
    plane of a model is derived once (``shading_coefficients``) and uploaded once for all views of the call."""
    from .device import DeviceArray

    def resident(model):
        return DeviceArray.from_host(shading_coefficients(model), device)

    coeff = resident(shading) if "flatfield" in shading else {k: resident(m) for k, m in shading.items()}
    return _apply_views(msims, [coeff] * len(msims), out_dtype, inplace, device, _shading_ops.apply_plane, "apply_shading")
