"""Plain numpy / scipy restatement of the tile intensity harmonisation (multiview_stitcher_amd.intensity, csrc/mvs_intensity.hip),
used by the tests as a checker only: float64 throughout, samples by scipy.ndimage.map_coordinates(order=1, mode="constant",
cval=nan) cast to float32 (as tests/psf_oracle.py samples), the cell rule of include/mvs_hip.h, a dense solve of the objective,
and the apply arithmetic in numpy float32 with the operation order the header gives.  The package is never called from here; the
overlap geometry comes from tests/metrics_oracle.py.

A view is the dict of tests/metrics_oracle.py: ``{"data", "origin", "spacing", "affines": {key: matrix}}``."""
import numpy as np
from scipy import ndimage

from oracle import fuse_oracle as fo
from tests import metrics_oracle as mo

MAX_CELLS = 16


# ---- the cell rule ----------------------------------------------------------------------------------------------------------------
def cell_of(c, g, n):
    return np.clip(np.floor((np.asarray(c, dtype=np.float64) + 0.5) * float(g) / float(n)), 0, g - 1).astype(np.int64)


def centres(g, n):
    return (np.arange(g, dtype=np.float64) + 0.5) * float(n) / float(g) - 0.5


def cell_edges(g, n):
    """Coordinates where the cell changes: k * n / g - 0.5 for k = 1 .. g - 1."""
    return np.arange(1, g, dtype=np.float64) * float(n) / float(g) - 0.5


# ---- samples and moments per cell pair --------------------------------------------------------------------------------------------
def grid_coords(affine, grid_shape):
    """(ndim, *grid_shape) pixel coordinates of every grid voxel: ((z m0 + y m1) + x m2) + offset, summed in that order."""
    matrix, offset = np.asarray(affine[0], dtype=np.float64), np.asarray(affine[1], dtype=np.float64)
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in grid_shape], indexing="ij")
    out = []
    for ax in range(len(grid_shape)):
        c = idx[0] * matrix[ax, 0]
        for k in range(1, len(grid_shape)):
            c = c + idx[k] * matrix[ax, k]
        out.append(c + offset[ax])
    return np.array(out)


def sample(data, coords):
    """Linear float32 samples of ``data`` at ``coords``; NaN out of bounds."""
    return ndimage.map_coordinates(np.asarray(data).astype(np.float32), coords, order=1, mode="constant", cval=np.nan).astype(np.float32)


def labelled_samples(fixed, moving, fixed_affine, moving_affine, grid_shape, cells_f, cells_m, halfspaces=None):
    """Per grid voxel: counted (bool), the two samples, and the cell multi-indices (ndim, *grid) of both tiles."""
    cf, cm = grid_coords(fixed_affine, grid_shape), grid_coords(moving_affine, grid_shape)
    f, m = sample(fixed, cf), sample(moving, cm)
    ok = np.isfinite(f) & np.isfinite(m)
    if halfspaces is not None and len(halfspaces):
        ok &= mo.index_mask(halfspaces, grid_shape)
    lab_f = np.array([cell_of(cf[ax], cells_f[ax], fixed.shape[ax]) for ax in range(len(grid_shape))])
    lab_m = np.array([cell_of(cm[ax], cells_m[ax], moving.shape[ax]) for ax in range(len(grid_shape))])
    return ok, f, m, lab_f, lab_m


def cell_pair_moments(fixed, moving, fixed_affine, moving_affine, grid_shape, cells_f, cells_m, halfspaces=None):
    """{(cell_f, cell_m): (n, mean_f, mean_m, M2_f, M2_m, C_fm)} over the cell pairs that hold at least one counted sample."""
    ok, f, m, lab_f, lab_m = labelled_samples(fixed, moving, fixed_affine, moving_affine, grid_shape, cells_f, cells_m, halfspaces)
    key_f = np.ravel_multi_index(tuple(lab_f), cells_f)
    key_m = np.ravel_multi_index(tuple(lab_m), cells_m)
    out = {}
    for kf in np.unique(key_f[ok]):
        for km in np.unique(key_m[ok & (key_f == kf)]):
            sel = ok & (key_f == kf) & (key_m == km)
            out[(tuple(int(v) for v in np.unravel_index(kf, cells_f)), tuple(int(v) for v in np.unravel_index(km, cells_m)))] = mo.moments(f[sel], m[sel])
    return out


def edge_clearance(fixed, moving, fixed_affine, moving_affine, grid_shape, cells_f, cells_m):
    """Smallest distance (pixels) of any grid voxel's coordinate, in either tile, to a cell edge or to the tile borders 0 and n - 1."""
    best = np.inf
    for data, affine, cells in ((fixed, fixed_affine, cells_f), (moving, moving_affine, cells_m)):
        c = grid_coords(affine, grid_shape)
        for ax in range(len(grid_shape)):
            marks = np.concatenate([[0.0, data.shape[ax] - 1.0], cell_edges(cells[ax], data.shape[ax])])
            best = min(best, np.abs(c[ax][..., None] - marks).min())
    return best


# ---- the objective ------------------------------------------------------------------------------------------------------------------
def solve(cells, records, lambda_identity=0.05, lambda_smooth=0.1, min_samples=64, reference_view=None, normalize=True):
    """Dense minimiser of the objective of intensity.fit_maps.  ``records``: (view_f, view_m, cell_f, cell_m, moments).  Returns
    (maps float64 ``cells_v + (2,)``, info) with info = {"s", "N", "before", "after"} (the data term at the identity / solution) and,
    for error bounds, the data term's matrix "D" over the unknowns (a, b / s per cell), the mask "free" and "w_identity"."""
    cells = [tuple(cv) for cv in cells]
    starts = np.cumsum([0] + [int(np.prod(cv)) for cv in cells])
    nc = int(starts[-1])
    recs = [(vf, vm, cf, cm, np.asarray(m, dtype=np.float64)) for vf, vm, cf, cm, m in records if m[0] >= min_samples and m[0] > 0]
    maps = [np.zeros(cv + (2,)) for cv in cells]
    for mp in maps:
        mp[..., 0] = 1.0
    info = {"s": 1.0, "N": 0.0, "before": 0.0, "after": 0.0}
    if recs:
        # second-moment matrix of (f, 1, m, 1) per record, from the six moments
        def second_moments(m):
            n, mf, mm, m2f, m2m, cfm = m
            sf, sm = n * mf, n * mm
            sff, smm, sfm = m2f + n * mf * mf, m2m + n * mm * mm, cfm + n * mf * mm
            return np.array([[sff, sf, sfm, sf], [sf, n, sm, n], [sfm, sm, smm, sm], [sf, n, sm, n]])

        N = float(sum(m[0] for *_, m in recs))
        s = float(np.sqrt(sum(second_moments(m)[0, 0] + second_moments(m)[2, 2] for *_, m in recs) / (2 * N)))
        s = s if s > 0 else 1.0
        scale = np.array([1.0 / s, 1.0, 1.0 / s, 1.0])          # unknowns (a, b / s): the samples in units of s
        sign = np.array([1.0, 1.0, -1.0, -1.0])
        H = np.zeros((2 * nc, 2 * nc))
        r = np.zeros(2 * nc)
        D = np.zeros((2 * nc, 2 * nc))                          # the data term alone
        for vf, vm, cf, cm, m in recs:
            kf = starts[vf] + np.ravel_multi_index(cf, cells[vf])
            km = starts[vm] + np.ravel_multi_index(cm, cells[vm])
            idx = [2 * kf, 2 * kf + 1, 2 * km, 2 * km + 1]
            S = second_moments(m)
            for i in range(4):
                for j in range(4):
                    D[idx[i], idx[j]] += sign[i] * sign[j] * scale[i] * scale[j] * S[i, j]
        H += D
        w_id, w_sm = lambda_identity * N / nc, lambda_smooth * N / nc
        for k in range(nc):
            H[2 * k, 2 * k] += w_id
            H[2 * k + 1, 2 * k + 1] += w_id
            r[2 * k] += w_id
        for v, cv in enumerate(cells):
            for cell in np.ndindex(*cv):
                for ax in range(len(cv)):
                    if cell[ax] + 1 < cv[ax]:
                        other = cell[:ax] + (cell[ax] + 1,) + cell[ax + 1:]
                        p = starts[v] + np.ravel_multi_index(cell, cv)
                        q = starts[v] + np.ravel_multi_index(other, cv)
                        for comp in (0, 1):
                            i, j = 2 * p + comp, 2 * q + comp
                            H[i, i] += w_sm
                            H[j, j] += w_sm
                            H[i, j] -= w_sm
                            H[j, i] -= w_sm
        u = np.zeros(2 * nc)
        u[0::2] = 1.0
        ident = u.copy()
        free = np.ones(2 * nc, dtype=bool)
        if reference_view is not None:
            free[2 * starts[reference_view]:2 * starts[reference_view + 1]] = False
        u[free] = np.linalg.solve(H[np.ix_(free, free)], r[free] - H[np.ix_(free, ~free)] @ u[~free])
        info = {"s": s, "N": N, "before": float(ident @ D @ ident), "after": float(u @ D @ u), "D": D, "free": free, "w_identity": w_id}
        for v, cv in enumerate(cells):
            maps[v] = u[2 * starts[v]:2 * starts[v + 1]].reshape(cv + (2,)).copy()
            maps[v][..., 1] *= s
    if normalize and reference_view is None:
        alpha = 1.0 / np.mean(np.concatenate([m[..., 0].ravel() for m in maps]))
        beta = -alpha * np.mean(np.concatenate([m[..., 1].ravel() for m in maps]))
        maps = [np.stack([alpha * m[..., 0], alpha * m[..., 1] + beta], axis=-1) for m in maps]
    return maps, info


def pair_grid(view_f, view_m, key, step=1):
    """Grid shape, the two grid index -> pixel maps and the halfspaces (grid index) of one pair: the geometry of
    metrics.tile_pair_image_metrics (tests/metrics_oracle.py) with a spacing of ``step`` fixed pixels; None without an overlap."""
    edge = mo.overlap_bboxes(view_f, view_m, key, None)
    if edge["lower"] is None or np.any(edge["lower"] >= edge["upper"]):
        return None
    ndim = view_f["data"].ndim
    of, sf = fo.coords_origin_spacing(view_f["origin"], view_f["spacing"], view_f["data"].shape)
    om, sm = fo.coords_origin_spacing(view_m["origin"], view_m["spacing"], view_m["data"].shape)
    sp = sf * float(step)
    lower, upper = edge["lower"], edge["upper"]
    shape = tuple(max(1, int(np.floor((upper[k] - lower[k]) / sp[k] + 1))) for k in range(ndim))
    out_bb = {"origin": np.array([float(v) for v in lower]), "spacing": sp, "shape": shape}
    eqs = np.array(edge["halfspaces"])
    eqs[:, -1] -= 1e-3 * np.min(sf)
    normals, c = eqs[:, :-1], eqs[:, -1]
    hs = np.concatenate([normals * sp[None, :], (normals @ out_bb["origin"] + c)[:, None]], axis=1)
    p_moving = np.linalg.inv(view_m["affines"][key]) @ view_f["affines"][key]
    return {"grid_shape": shape, "halfspaces": hs, "fixed_affine": fo.transform_params(np.eye(ndim + 1), of, sf, out_bb),
            "moving_affine": fo.transform_params(p_moving, om, sm, out_bb)}


def fit_maps(views, key, cells, pairs, step=1, **solver):
    """intensity.fit_maps on plain views: (maps float64, info).  ``cells``: one tuple for all views; ``pairs``: (i, j), i < j."""
    per_view = [tuple(cells)] * len(views)
    records = []
    for i, j in pairs:
        g = pair_grid(views[i], views[j], key, step)
        if g is None:
            continue
        mom = cell_pair_moments(views[i]["data"], views[j]["data"], g["fixed_affine"], g["moving_affine"], g["grid_shape"], per_view[i],
                                per_view[j], g["halfspaces"])
        records.extend((i, j, cf, cm, m) for (cf, cm), m in mom.items())
    return solve(per_view, records, **solver)


# ---- apply --------------------------------------------------------------------------------------------------------------------------
def axis_table(n, g):
    """Lower cell and weight per pixel index: the coordinate clamped to the first and last centre, in units of the centre spacing."""
    if g == 1:
        return np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float32)
    c = centres(g, n)
    u = (np.clip(np.arange(n, dtype=np.float64), c[0], c[-1]) - c[0]) / (float(n) / float(g))
    lower = np.clip(np.floor(u), 0, g - 2)
    return lower.astype(np.int64), (u - lower).astype(np.float32)


def lerp32(u, v, t):
    u, v, t = (np.asarray(q, dtype=np.float32) for q in (u, v, t))
    d = (v - u).astype(np.float32)
    return (u + (t * d).astype(np.float32)).astype(np.float32)


def apply(data, coeff, out_dtype=None):
    """a(p) * data + b(p) in float32 with the operation order of mvs_intensity_apply: the coefficient pairs interpolated along z,
    then y (per row), then x (per voxel), then the product and the sum; integer outputs rounded half to even and saturated."""
    data = np.asarray(data)
    coeff = np.asarray(coeff, dtype=np.float32)
    out_dtype = data.dtype if out_dtype is None else np.dtype(out_dtype)
    ndim = data.ndim
    shape = (1,) * (3 - ndim) + data.shape
    cells = (1,) * (3 - ndim) + coeff.shape[:-1]
    C = coeff.reshape(cells + (2,))
    x = data.reshape(shape).astype(np.float32)
    (iz, tz), (iy, ty), (ix, tx) = [axis_table(n, g) for n, g in zip(shape, cells)]
    iz1, iy1, ix1 = np.minimum(iz + 1, cells[0] - 1), np.minimum(iy + 1, cells[1] - 1), np.minimum(ix + 1, cells[2] - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        # rows: (nz, ny, gx, 2)
        tzb, tyb = tz[:, None, None, None], ty[None, :, None, None]
        r0 = lerp32(C[iz][:, iy], C[iz1][:, iy], np.broadcast_to(tzb, (shape[0], shape[1], cells[2], 2)))
        r1 = lerp32(C[iz][:, iy1], C[iz1][:, iy1], np.broadcast_to(tzb, (shape[0], shape[1], cells[2], 2)))
        row = lerp32(r0, r1, np.broadcast_to(tyb, r0.shape))
        ab = lerp32(row[:, :, ix], row[:, :, ix1], np.broadcast_to(tx[None, None, :, None], (shape[0], shape[1], shape[2], 2)))
        y = ((ab[..., 0] * x).astype(np.float32) + ab[..., 1]).astype(np.float32)
        if out_dtype.kind == "f":
            return y.reshape(data.shape)
        vmax = np.float32(np.iinfo(out_dtype).max)
        r = np.rint(y)
        r = np.where(r >= 0, r, np.float32(0))
        r = np.where(r > vmax, vmax, r)
    return r.astype(out_dtype).reshape(data.shape)
