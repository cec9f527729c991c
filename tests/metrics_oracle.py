"""Plain numpy / scipy restatement of the reference's registration quality metrics (src/multiview_stitcher/metrics.py) and of the
halfspace helpers it uses (mv_graph.py, registration._get_overlap_bboxes), independent of the package.

A view is a dict ``{"data": spatial ndarray, "origin": (ndim,), "spacing": (ndim,), "affines": {key: (ndim + 1, ndim + 1)}}``; axes are
the last ``ndim`` of (z, y, x).  Sampling goes through ``oracle.fuse_oracle.transform_array(order=1, cval=nan)`` (scipy.ndimage.
affine_transform with the parameters of transformation.py:37-83) and the NCC is the reference's two-pass float64.  ``sample_dtype``
is the dtype the tiles are cast to before they are resampled: float32 is what the reference does (metrics.py:713, 729; scipy
interpolates in double and rounds each output sample once), float64 keeps the samples unrounded.
"""
import numpy as np
from scipy.ndimage import affine_transform
from scipy.optimize import linprog
from scipy.spatial import ConvexHull, HalfspaceIntersection, QhullError

from oracle import fuse_oracle as fo

SDIMS = ["z", "y", "x"]


# ---- metrics.py:42-79 ---------------------------------------------------------------------------------------------------
def normalized_cross_correlation(im1, im2):
    a = np.asarray(im1, dtype=np.float64)
    b = np.asarray(im2, dtype=np.float64)
    mask = ~(np.isnan(a) | np.isnan(b))
    if np.sum(mask) < 2:
        return np.nan
    a = a[mask]
    b = b[mask]
    a_c = a - a.mean()
    b_c = b - b.mean()
    denom = np.sqrt(np.sum(a_c**2) * np.sum(b_c**2))
    if denom < 1e-10:
        return np.nan
    return float(np.dot(a_c, b_c) / denom)


def moments(fixed, moving):
    """(n, mean_f, mean_m, M2_f, M2_m, C_fm) of the positions where both arrays are finite: two passes in float64."""
    a = np.asarray(fixed, dtype=np.float64).ravel()
    b = np.asarray(moving, dtype=np.float64).ravel()
    ok = np.isfinite(a) & np.isfinite(b)
    n = int(ok.sum())
    if n == 0:
        return np.zeros(6)
    a, b = a[ok], b[ok]
    a_c, b_c = a - a.mean(), b - b.mean()
    return np.array([n, a.mean(), b.mean(), np.sum(a_c**2), np.sum(b_c**2), np.dot(a_c, b_c)])


# ---- stack properties and halfspaces (mv_graph.py:183-218, 301-338, 386-420, 475-493; spatial_image_utils.py:889-913) --------
def stack_props(view, key=None):
    data = view["data"]
    origin, spacing = fo.coords_origin_spacing(view["origin"], view["spacing"], data.shape)
    sp = {"shape": np.array(data.shape), "spacing": spacing, "origin": origin}
    if key is not None:
        sp["transform"] = np.asarray(view["affines"][key], dtype=np.float64)
    return sp


def extend_stack_props(sp, extend_by):
    """spatial_image_utils.extend_stack_props: ``extend_by`` a scalar or an (ndim,) array; negative values shrink."""
    ext = np.broadcast_to(np.asarray(extend_by, dtype=np.float64), sp["origin"].shape)
    out = dict(sp)
    out["shape"] = sp["shape"] + np.ceil(2 * ext / sp["spacing"]).astype(int)
    out["origin"] = sp["origin"] - ext
    return out


def faces(sp):
    ndim = len(sp["origin"])
    gv = np.array(list(np.ndindex(*([2] * ndim))))
    f = np.array([gv[gv[:, ax] == side] for ax in range(ndim) for side in (0, 1)])
    f = f * (sp["shape"] - 1) * sp["spacing"] + sp["origin"]
    if "transform" in sp:
        shp = f.shape
        pts = np.hstack([f.reshape(-1, ndim), np.ones((f.size // ndim, 1))])
        f = np.dot(sp["transform"], pts.T).T[:, :-1].reshape(shp)
    return f


def center(sp):
    ndim = len(sp["origin"])
    c = sp["origin"] + sp["spacing"] * (sp["shape"] - 1) / 2
    if "transform" in sp:
        c = np.matmul(sp["transform"], np.concatenate([c, np.ones(1)]))[:ndim]
    return c


def halfspace_equations(sp):
    """Rows [n, c] with n . x + c <= 0 inside the stack (mv_graph.py:183-218)."""
    fs, ctr = faces(sp), center(sp)
    ndim = fs.shape[-1]
    eqs = []
    for face in fs:
        if ndim == 2:
            normal = np.array([-(face[1][1] - face[0][1]), face[1][0] - face[0][0]])
        else:
            normal = np.cross(face[1] - face[0], face[2] - face[0])
        normal = normal / np.linalg.norm(normal)
        c = -np.dot(normal, face[0])
        if np.dot(normal, ctr) + c > 0:
            normal = -normal
        c = -np.dot(normal, face[0])
        eqs.append(np.concatenate([normal, [c]]))
    return np.array(eqs)


def overlap_between(sp1, sp2):
    """(volume, HalfspaceIntersection) of two stacks, (-1, None) without an intersection (mv_graph.py:301-338)."""
    eqs = np.concatenate([halfspace_equations(sp1), halfspace_equations(sp2)])
    norm = np.reshape(np.linalg.norm(eqs[:, :-1], axis=1), (eqs.shape[0], 1))
    c = np.zeros((eqs.shape[1],))
    c[-1] = -1
    res = linprog(c, A_ub=np.hstack((eqs[:, :-1], norm)), b_ub=-eqs[:, -1:], bounds=(None, None))
    if res.x is None:
        return -1, None
    try:
        hs = HalfspaceIntersection(eqs, res.x[:-1])
    except QhullError:
        return -1, None
    return ConvexHull(hs.intersections).volume, hs


def transform_pts(pts, affine):
    pts = np.concatenate([np.asarray(pts, dtype=np.float64), np.ones((len(pts), 1))], axis=1)
    return np.dot(pts, np.asarray(affine).T)[:, :-1]


def world_box(sp):
    """(lo, hi) of a stack whose transform is a positive diagonal scaling plus a shift, else None."""
    ndim = len(sp["origin"])
    lin = sp["transform"][:ndim, :ndim]
    if np.any(lin - np.diag(np.diag(lin)) != 0) or np.any(np.diag(lin) <= 0):
        return None
    lo = sp["origin"]
    hi = lo + (sp["shape"] - 1) * sp["spacing"]
    return np.diag(lin) * lo + sp["transform"][:ndim, ndim], np.diag(lin) * hi + sp["transform"][:ndim, ndim]


def overlap_bboxes(view1, view2, key, tol, exact_corners=True):
    """registration._get_overlap_bboxes(sim1, sim2, key, None, tol) (registration.py:194-277) for sim1: lower / upper of the
    intersection vertices in view1's intrinsic space, the halfspace equations there (mv_graph.transform_halfspace, mv_graph.py:293)
    and the overlap volume; ``None`` entries without an intersection.

    ``exact_corners``: the reference takes the vertices from Qhull, which are off by a few ulp; where upper - lower is a whole
    number of pixels -- every stage-positioned mosaic -- that decides whether ``floor((upper - lower) / spacing + 1)`` keeps the last
    row (observed: 46.99999999999999 for an overlap of 48 rows, so 47 rows).  The package's specification asks for the exact box, so
    by default two axis-aligned views get the corners of the intersection of their boxes; ``False`` is the reference as it stands."""
    sps = [stack_props(v, key) for v in (view1, view2)]
    if tol is not None:
        sps = [extend_stack_props(sp, tol) for sp in sps]
    vol, hs = overlap_between(sps[0], sps[1])
    if hs is None:
        return {"lower": None, "upper": None, "halfspaces": None, "vol": vol}
    T1 = np.asarray(view1["affines"][key], dtype=np.float64)
    vertices = hs.intersections
    boxes = [world_box(sp) for sp in sps]
    if exact_corners and boxes[0] is not None and boxes[1] is not None:
        lo, hi = np.maximum(boxes[0][0], boxes[1][0]), np.minimum(boxes[0][1], boxes[1][1])
        vertices = np.array(list(np.ndindex(*([2] * len(lo))))) * (hi - lo) + lo
    corners = transform_pts(vertices, np.linalg.inv(T1))
    return {"lower": np.min(corners, axis=0), "upper": np.max(corners, axis=0),
            "halfspaces": hs.halfspaces @ np.linalg.inv(np.linalg.inv(T1)), "vol": vol}


def mask_from_halfspace(coord_arrays, eqs):
    """mv_graph.get_mask_from_halfspace (mv_graph.py:542-581) over the physical coordinates of a grid."""
    grids = np.meshgrid(*coord_arrays, indexing="ij")
    pts = np.stack([g.ravel() for g in grids], axis=-1)
    vals = pts @ eqs[:, :-1].T + eqs[:, -1]
    return np.all(vals <= 0, axis=-1).reshape(tuple(len(c) for c in coord_arrays))


def halfspace_distances(coord_arrays, eqs):
    """|n . x + c| of the grid point closest to any plane (the test's input condition: no voxel on a plane)."""
    grids = np.meshgrid(*coord_arrays, indexing="ij")
    pts = np.stack([g.ravel() for g in grids], axis=-1)
    return np.abs(pts @ eqs[:, :-1].T + eqs[:, -1]).min()


# ---- the pixel-level form the kernel takes --------------------------------------------------------------------------------------
def sample(data, matrix, offset, shape, sample_dtype=np.float32):
    """scipy.ndimage.affine_transform(order=1, mode="constant", cval=nan) of ``data`` cast to ``sample_dtype``."""
    return affine_transform(np.asarray(data).astype(sample_dtype), matrix=np.asarray(matrix), offset=np.asarray(offset), output_shape=tuple(shape),
                            mode="constant", cval=np.nan, order=1)


def index_mask(grid_eqs, shape):
    """The halfspace mask over grid INDEX coordinates: rows (a.., b), a . index + b <= 0."""
    return mask_from_halfspace([np.arange(n, dtype=np.float64) for n in shape], np.asarray(grid_eqs, dtype=np.float64))


def pair_moments(fixed, moving, fixed_affine, cand_affines, grid_shape, halfspaces=None, device=0, sample_dtype=np.float32):
    """What mvs_pair_moments computes, from scipy's samples: the stand-in of ``_metric_ops.pair_moments`` on the CPU."""
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    f = np.array(sample(fixed, fixed_affine[0], fixed_affine[1], grid_shape, sample_dtype), dtype=np.float64)
    if halfspaces is not None and len(halfspaces):
        f[~index_mask(halfspaces, grid_shape)] = np.nan
    return np.array([moments(f, sample(moving, m, o, grid_shape, sample_dtype)) for m, o in cand_affines]).reshape(-1, 6)


def sample_border_distance(matrix, offset, grid_shape, data_shape):
    """Smallest distance (pixels) of any grid voxel's coordinate to the tile's borders 0 and n - 1 along any axis."""
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in grid_shape], indexing="ij"), axis=-1).reshape(-1, len(grid_shape))
    c = idx @ np.asarray(matrix).T + np.asarray(offset)
    hi = np.asarray(data_shape, dtype=np.float64) - 1
    return min(np.abs(c).min(), np.abs(c - hi).min())


# ---- metrics.py:127-379, 387-808 -----------------------------------------------------------------------------------------------
def _tolerance(max_tolerance, ndim):
    if max_tolerance is None:
        return None
    if isinstance(max_tolerance, (int, float)):
        return -float(max_tolerance)
    return np.array([-float(max_tolerance.get(d, 0.0)) for d in SDIMS[-ndim:]])


def adjacency_edges(views, key, tol):
    """Edges of mv_graph.build_view_adjacency_graph_from_msims (mv_graph.py:35-180): the pairs with a positive overlap volume.
    Every pair is tried (the reference's ball query only leaves out pairs that cannot overlap)."""
    sps = [stack_props(v, key) for v in views]
    if tol is not None:
        sps = [extend_stack_props(sp, tol) for sp in sps]
    return [(i, j) for i in range(len(views)) for j in range(i + 1, len(views)) if overlap_between(sps[i], sps[j])[0] > 0]


def metrics_edges(views, base_key, query_keys, pairs_graph, max_tolerance, bidirectional):
    """[( (fixed, moving), {"lower", "upper", "halfspaces", "vol", "transforms"} )] in the order of DiGraph.edges()."""
    ndim = views[0]["data"].ndim
    tol = _tolerance(max_tolerance, ndim)
    out = []
    if pairs_graph is None:
        for i, j in adjacency_edges(views, base_key, tol):
            for f, m in ([(i, j), (j, i)] if bidirectional else [(min(i, j), max(i, j))]):
                e = overlap_bboxes(views[f], views[m], base_key, tol)
                e["transforms"] = {q: np.linalg.inv(views[m]["affines"][q]) @ views[f]["affines"][q] for q in query_keys}
                out.append(((f, m), e))
    else:
        for (i, j), T_edge in pairs_graph.items():
            fb, mb = min(i, j), max(i, j)
            T_edge = np.asarray(T_edge, dtype=np.float64)
            for f, m in ([(fb, mb), (mb, fb)] if bidirectional else [(fb, mb)]):
                e = overlap_bboxes(views[f], views[m], base_key, tol)
                T_fixed_base, T_moving_base = views[f]["affines"][base_key], views[m]["affines"][base_key]
                if f < m:
                    p_moving = np.linalg.inv(T_moving_base) @ T_edge @ T_fixed_base
                else:       # metrics.py:367-368, as it stands
                    p_moving = np.linalg.inv(T_fixed_base) @ np.linalg.inv(T_edge) @ T_moving_base
                e["transforms"] = {"transform": p_moving}
                out.append(((f, m), e))
    return sorted(out, key=lambda e: e[0][0])


def pair_arrays(view_f, view_m, edge, q, spacing=None, sample_dtype=np.float32):
    """The two arrays metrics._compute_metrics_from_arrays hands the metric functions for candidate ``q`` of one directed edge
    (metrics.py:627-630, 674-742, 111-124): float arrays with NaN outside the tiles, the fixed one NaN outside the halfspaces."""
    ndim = view_f["data"].ndim
    _, fixed_spacing = fo.coords_origin_spacing(view_f["origin"], view_f["spacing"], view_f["data"].shape)
    eqs = np.array(edge["halfspaces"])
    eqs[:, -1] -= 1e-3 * np.min(fixed_spacing)
    sp = fixed_spacing if spacing is None else np.array([float(spacing[d]) for d in SDIMS[-ndim:]])
    lower, upper = edge["lower"], edge["upper"]
    shape = [max(1, int(np.floor((upper[k] - lower[k]) / sp[k] + 1))) for k in range(ndim)]
    out_bb = {"origin": np.array([float(v) for v in lower]), "spacing": sp, "shape": shape}
    origins = [fo.coords_origin_spacing(v["origin"], v["spacing"], v["data"].shape) for v in (view_f, view_m)]
    fixed = np.array(fo.transform_array(view_f["data"].astype(sample_dtype), np.eye(ndim + 1), origins[0][0], origins[0][1], out_bb, order=1, cval=np.nan))
    moving = fo.transform_array(view_m["data"].astype(sample_dtype), edge["transforms"][q], origins[1][0], origins[1][1], out_bb, order=1, cval=np.nan)
    coords = [out_bb["origin"][k] + sp[k] * np.arange(shape[k], dtype=float) for k in range(ndim)]
    fixed[~mask_from_halfspace(coords, eqs)] = np.nan
    return fixed, moving


def tile_pair_image_metrics(views, base_key, query_keys=None, metric_funcs=None, max_tolerance=None, spacing=None, bidirectional=False,
                            pairs_graph=None, sample_dtype=np.float32):
    """metrics.tile_pair_image_metrics on plain views at one resolution level.  ``pairs_graph``: {(i, j): world-space transform}."""
    if (query_keys is None) == (pairs_graph is None):
        raise ValueError("Exactly one of 'query_transform_keys' or 'pairs_graph' must be provided.")
    if metric_funcs is None:
        metric_funcs = {"ncc": normalized_cross_correlation}
    if isinstance(query_keys, str):
        query_keys = [query_keys]
    candidate_keys = list(query_keys) if query_keys is not None else ["transform"]
    edges = metrics_edges(views, base_key, candidate_keys, pairs_graph, max_tolerance, bidirectional)
    computed, bboxes, vols = {}, {}, {}
    for (f, m), e in edges:
        vols[(f, m)] = e["vol"]
        if e["lower"] is None or np.any(e["lower"] >= e["upper"]):
            bboxes[(f, m)] = None
            computed[(f, m)] = {q: {k: np.nan for k in metric_funcs} for q in candidate_keys}
            continue
        bboxes[(f, m)] = {"lower": e["lower"], "upper": e["upper"]}
        computed[(f, m)] = {}
        for q in candidate_keys:
            fa, ma = pair_arrays(views[f], views[m], e, q, spacing, sample_dtype)
            fa32, ma32 = (fa, ma) if sample_dtype == np.float64 else (np.asarray(fa, dtype=np.float32), np.asarray(ma, dtype=np.float32))
            computed[(f, m)][q] = {k: float(func(fa32, ma32)) for k, func in metric_funcs.items()}
    summary = {}
    for q in candidate_keys:
        summary[q] = {}
        for key in metric_funcs:
            valid = [(computed[p][q][key], float(vols[p])) for p in computed if not np.isnan(computed[p][q][key])]
            total = sum(w for _, w in valid)
            summary[q][key] = float(sum(v * w for v, w in valid) / total) if valid and total > 0 else np.nan
    return {"pairs": computed, "bboxes": bboxes, "summary": summary}
