"""Plain numpy / scipy restatement of the non-rigid tile refinement (multiview_stitcher_amd.nonrigid, csrc/mvs_nonrigid.hip), used by
the tests as a checker only: float64 throughout, samples by scipy.ndimage.map_coordinates(order=1), the block moments by two-pass
sums, the peak search and the objective by plain loops, the warp with the field interpolated in numpy float32 in the operation order
the header gives and the value sampled in float64.  The package is never called from here; the overlap geometry, the cell rule and
the float32 lerp come from tests/intensity_oracle.py and tests/metrics_oracle.py.

A view is the dict of tests/metrics_oracle.py: ``{"data", "origin", "spacing", "affines": {key: matrix}}``."""
import numpy as np
from scipy import ndimage

from tests import intensity_oracle as io
from tests import metrics_oracle as mo

REASONS = ("few_samples", "low_ncc", "rim", "flat")


# ---- block moments ----------------------------------------------------------------------------------------------------------------
def box_coords(affine, lo, hi):
    """(ndim, *(hi - lo)) pixel coordinates of the grid indices lo <= index < hi: ((z m0 + y m1) + x m2) + offset, in that order."""
    matrix, offset = np.asarray(affine[0], dtype=np.float64), np.asarray(affine[1], dtype=np.float64)
    idx = np.meshgrid(*[np.arange(a, b, dtype=np.float64) for a, b in zip(lo, hi)], indexing="ij")
    out = []
    for ax in range(len(lo)):
        c = idx[0] * matrix[ax, 0]
        for k in range(1, len(lo)):
            c = c + idx[k] * matrix[ax, k]
        out.append(c + offset[ax])
    return np.array(out), idx


def box_samples(data, affine, lo, hi, halfspaces=None, sample_dtype=np.float32):
    """Linear samples of ``data`` (cast to float32 first, rounded to ``sample_dtype``) at the grid indices of the box, NaN out of
    bounds, where the sample is not finite and -- with ``halfspaces`` -- where one of them does not hold at the index."""
    coords, idx = box_coords(affine, lo, hi)
    v = ndimage.map_coordinates(np.asarray(data).astype(np.float32).astype(np.float64), coords, order=1, mode="constant", cval=np.nan)
    v = v.astype(sample_dtype).astype(np.float64)
    v[~np.isfinite(v)] = np.nan
    if halfspaces is not None and len(halfspaces):
        for row in np.asarray(halfspaces, dtype=np.float64):
            acc = idx[0] * row[0]
            for k in range(1, len(lo)):
                acc = acc + idx[k] * row[k]
            v[~(acc + row[-1] <= 0.0)] = np.nan
    return v


def halfspace_clearance(blocks, halfspaces):
    """|a . g + b| of the block voxel closest to any plane (the input condition of exact counts)."""
    blocks = np.asarray(blocks)
    lo, hi = blocks[:, 0].min(axis=0), (blocks[:, 0] + blocks[:, 1]).max(axis=0)
    return mo.halfspace_distances([np.arange(a, b, dtype=np.float64) for a, b in zip(lo, hi)], np.asarray(halfspaces, dtype=np.float64))


def border_clearance(affine, blocks, radius, shape):
    """Smallest distance (pixels) of a coordinate of the blocks grown by ``radius`` to the tile borders 0 and n - 1."""
    blocks = np.asarray(blocks)
    r = np.asarray(radius)
    coords, _ = box_coords(affine, blocks[:, 0].min(axis=0) - r, (blocks[:, 0] + blocks[:, 1]).max(axis=0) + r)
    return min(min(np.abs(coords[ax]).min(), np.abs(coords[ax] - (shape[ax] - 1.0)).min()) for ax in range(len(shape)))


def block_samples(fixed, moving, fixed_affine, moving_affine, blocks, radius, halfspaces=None, sample_dtype=np.float32):
    """(F, M, lo): the fixed samples over the bounding box of all blocks and the moving samples over that box grown by ``radius``."""
    blocks = np.asarray(blocks, dtype=np.int64)
    r = np.asarray(radius, dtype=np.int64)
    lo, hi = blocks[:, 0].min(axis=0), (blocks[:, 0] + blocks[:, 1]).max(axis=0)
    return (box_samples(fixed, fixed_affine, lo, hi, halfspaces, sample_dtype), box_samples(moving, moving_affine, lo - r, hi + r, None, sample_dtype), lo)


def moments_of_samples(F, M, lo, blocks, radius):
    blocks = np.asarray(blocks, dtype=np.int64)
    r = [int(v) for v in radius]
    shifts = list(np.ndindex(*[2 * v + 1 for v in r]))
    out = np.zeros((len(blocks), len(shifts), 6))
    for b, blk in enumerate(blocks):
        a, n = blk[0] - lo, blk[1]
        f = F[tuple(slice(a[k], a[k] + n[k]) for k in range(len(r)))]
        for s, sh in enumerate(shifts):                 # index sh[k] is the shift sh[k] - r[k]; M starts r[k] before F
            out[b, s] = mo.moments(f, M[tuple(slice(a[k] + sh[k], a[k] + sh[k] + n[k]) for k in range(len(r)))])
    return out


def block_moments(fixed, moving, fixed_affine, moving_affine, blocks, radius, halfspaces=None, sample_dtype=np.float32):
    """What mvs_block_match computes: (B, S, 6), rows (n, mean_f, mean_m, M2_f, M2_m, C_fm) over the pairs (f(g), m(g + s))."""
    F, M, lo = block_samples(fixed, moving, fixed_affine, moving_affine, blocks, radius, halfspaces, sample_dtype)
    return moments_of_samples(F, M, lo, blocks, radius)


# ---- shifts -------------------------------------------------------------------------------------------------------------------------
def ncc(row):
    n, _, _, m2f, m2m, cfm = (float(v) for v in row)
    if n < 2:
        return np.nan
    denom = np.sqrt(m2f * m2m)
    return np.nan if denom < 1e-10 else cfm / denom


def shifts_from_moments(moments, radius, min_samples=64, min_ncc=0.3):
    """Per block a dict: ``reason`` (None when kept), ``shift``, ``weight``, and for the margins of the tests ``peak``, ``runner_up``
    (the largest NCC elsewhere; -inf without one), ``n``, ``second`` (the second differences of the axes that were examined)."""
    r = [int(v) for v in radius]
    window = tuple(2 * v + 1 for v in r)
    out = []
    for rows in np.asarray(moments, dtype=np.float64):
        c = np.array([ncc(row) for row in rows])
        best = None
        for i, v in enumerate(c):                       # the first maximum in index order, NaNs left out
            if not np.isnan(v) and (best is None or v > c[best]):
                best = i
        if best is None:
            best = int(np.ravel_multi_index(r, window))
        others = [v for i, v in enumerate(c) if i != best and not np.isnan(v)]
        k = np.unravel_index(best, window)
        rec = {"reason": None, "shift": None, "weight": 0.0, "peak": c[best], "runner_up": max(others) if others else -np.inf, "n": rows[best, 0],
               "second": [], "index": k}
        cube = c.reshape(window)
        if rows[best, 0] < min_samples:
            rec["reason"] = "few_samples"
        elif np.isnan(c[best]) or c[best] < min_ncc:
            rec["reason"] = "low_ncc"
        elif any(r[ax] > 0 and (k[ax] == 0 or k[ax] == 2 * r[ax]) for ax in range(len(r))):
            rec["reason"] = "rim"
        else:
            s = np.zeros(len(r))
            for ax in range(len(r)):
                s[ax] = k[ax] - r[ax]
                if r[ax] == 0:
                    continue
                km, kp = list(k), list(k)
                km[ax] -= 1
                kp[ax] += 1
                cm, cp = cube[tuple(km)], cube[tuple(kp)]
                second = cm - 2.0 * c[best] + cp
                rec["second"].append(second)
                if np.isnan(cm) or np.isnan(cp) or not second < 0:
                    rec["reason"] = "flat"
                    break
                s[ax] += min(max(0.5 * (cm - cp) / second, -0.5), 0.5)
            if rec["reason"] is None:
                rec["shift"], rec["weight"] = s, rows[best, 0] * c[best]
        out.append(rec)
    return out


# ---- the objective ------------------------------------------------------------------------------------------------------------------
def solve(nodes, records, lambda_identity=0.05, lambda_smooth=0.1, reference_view=None):
    """Dense minimiser of the objective of nonrigid.fit_fields, one scalar solve per axis.  ``records``: (view_f, view_m, cell_f,
    cell_m, s_world, w).  Returns the world-unit vectors per view, float64 ``nodes_v + (ndim,)``."""
    nodes = [tuple(nv) for nv in nodes]
    ndim = len(nodes[0])
    starts = np.cumsum([0] + [int(np.prod(nv)) for nv in nodes])
    nc = int(starts[-1])
    W = float(sum(r[5] for r in records))
    u = np.zeros((nc, ndim))
    if W > 0:
        H = np.zeros((nc, nc))
        rhs = np.zeros((nc, ndim))
        for vf, vm, cf, cm, s, w in records:
            p = starts[vf] + np.ravel_multi_index(cf, nodes[vf])
            q = starts[vm] + np.ravel_multi_index(cm, nodes[vm])
            H[p, p] += w
            H[q, q] += w
            H[p, q] -= w
            H[q, p] -= w
            rhs[q] += w * np.asarray(s, dtype=np.float64)
            rhs[p] -= w * np.asarray(s, dtype=np.float64)
        w_id, w_sm = lambda_identity * W / nc, lambda_smooth * W / nc
        H[np.arange(nc), np.arange(nc)] += w_id
        for v, nv in enumerate(nodes):
            for cell in np.ndindex(*nv):
                for ax in range(ndim):
                    if cell[ax] + 1 < nv[ax]:
                        other = cell[:ax] + (cell[ax] + 1,) + cell[ax + 1:]
                        p = starts[v] + np.ravel_multi_index(cell, nv)
                        q = starts[v] + np.ravel_multi_index(other, nv)
                        H[p, p] += w_sm
                        H[q, q] += w_sm
                        H[p, q] -= w_sm
                        H[q, p] -= w_sm
        free = np.ones(nc, dtype=bool)
        if reference_view is not None:
            free[starts[reference_view]:starts[reference_view + 1]] = False
        for ax in range(ndim):
            u[free, ax] = np.linalg.solve(H[np.ix_(free, free)], rhs[free, ax])
    return [u[starts[v]:starts[v + 1]].reshape(nv + (ndim,)) for v, nv in enumerate(nodes)]


def objective(nodes, records, us, lambda_identity, lambda_smooth):
    """The value of the objective at the world-unit vectors ``us`` (per view ``nodes_v + (ndim,)``)."""
    nc = sum(int(np.prod(nv)) for nv in nodes)
    W = float(sum(r[5] for r in records))
    val = sum(w * np.sum((us[vm][tuple(cm)] - us[vf][tuple(cf)] - s) ** 2) for vf, vm, cf, cm, s, w in records)
    val += lambda_identity * W / nc * sum(np.sum(u ** 2) for u in us)
    for u in us:
        for ax in range(u.ndim - 1):
            val += lambda_smooth * W / nc * np.sum(np.diff(u, axis=ax) ** 2)
    return val


def plan_blocks(grid_shape, block, fixed_affine, moving_affine, shape_f, shape_m, nodes_f, nodes_m):
    """Rows (lo, n, cell_f, cell_m) per box of at most ``block`` per axis, C order, the cells from the box centre clamped into the tile."""
    out = []
    for pos in np.ndindex(*[-(-s // b) for s, b in zip(grid_shape, block)]):
        lo = np.array([p * b for p, b in zip(pos, block)])
        n = np.array([min(b, s - l) for b, s, l in zip(block, grid_shape, lo)])
        ctr = lo + (n - 1) / 2.0
        cells = []
        for affine, shape, nodes in ((fixed_affine, shape_f, nodes_f), (moving_affine, shape_m, nodes_m)):
            pix = np.asarray(affine[0], dtype=np.float64) @ ctr + np.asarray(affine[1], dtype=np.float64)
            cells.append([int(io.cell_of(min(max(pix[ax], 0.0), shape[ax] - 1.0), nodes[ax], shape[ax])) for ax in range(len(lo))])
        out.append([lo, n, cells[0], cells[1]])
    return np.array(out, dtype=np.int64)


def rms(records, residual=None):
    """Weighted RMS of |s_world| (or of the given residual vectors) over records."""
    w = np.array([r[5] for r in records])
    v = np.array([r[4] for r in records]) if residual is None else np.asarray(residual)
    return float(np.sqrt(np.sum(w * np.sum(v ** 2, axis=1)) / np.sum(w)))


def match_pairs(views, key, nodes, pairs, block, radius, step=1, min_samples=64, min_ncc=0.3, sample_dtype=np.float32):
    """Block matching of every pair: ({(i, j): (blocks, found)}, records) with ``found`` the rows of ``shifts_from_moments``."""
    ndim = views[0]["data"].ndim
    per_pair, records = {}, []
    for i, j in pairs:
        g = io.pair_grid(views[i], views[j], key, step)
        if g is None:
            continue
        blocks = plan_blocks(g["grid_shape"], block, g["fixed_affine"], g["moving_affine"], views[i]["data"].shape, views[j]["data"].shape, nodes, nodes)
        mom = block_moments(views[i]["data"], views[j]["data"], g["fixed_affine"], g["moving_affine"], blocks, radius, g["halfspaces"], sample_dtype)
        found = shifts_from_moments(mom, radius, min_samples, min_ncc)
        per_pair[(i, j)] = (blocks, found)
        L = views[i]["affines"][key][:ndim, :ndim]
        for b, f in zip(blocks, found):
            if f["reason"] is None:
                records.append((i, j, tuple(b[2]), tuple(b[3]), L @ (float(step) * np.asarray(views[i]["spacing"], dtype=np.float64) * f["shift"]), f["weight"]))
    return per_pair, records


def fit_fields(views, key, nodes, pairs, block, radius, step=1, min_samples=64, min_ncc=0.3, lambda_identity=0.05, lambda_smooth=0.1,
               reference_view=None, sample_dtype=np.float32):
    """nonrigid.fit_fields on plain views: (fields float64 in pixels, info).  ``nodes``: one tuple for all views."""
    ndim = views[0]["data"].ndim
    per_pair, records = match_pairs(views, key, nodes, pairs, block, radius, step, min_samples, min_ncc, sample_dtype)
    us = solve([tuple(nodes)] * len(views), records, lambda_identity, lambda_smooth, reference_view)
    fields = [u @ np.linalg.inv(v["affines"][key][:ndim, :ndim]).T / np.asarray(v["spacing"], dtype=np.float64) for u, v in zip(us, views)]
    res = [us[vm][tuple(cm)] - us[vf][tuple(cf)] - s for vf, vm, cf, cm, s, w in records]
    info = {"per_pair": per_pair, "records": records, "rms_before": rms(records) if records else np.nan,
            "rms_after": rms(records, res) if records else np.nan}
    return fields, info


# ---- warp ---------------------------------------------------------------------------------------------------------------------------
def displacement(shape, field):
    """The float32 displacement of every voxel, (*shape, ndim): the field interpolated along z, then y (per row), then x, with the
    lerp u + t (v - u) in float32 and the tables of the intensity maps."""
    field = np.asarray(field, dtype=np.float32)
    ndim = len(shape)
    shape3 = (1,) * (3 - ndim) + tuple(shape)
    nodes3 = (1,) * (3 - ndim) + field.shape[:-1]
    C = np.zeros(nodes3 + (3,), np.float32)
    C[..., 3 - ndim:] = field.reshape(nodes3 + (ndim,))
    (iz, tz), (iy, ty), (ix, tx) = [io.axis_table(n, g) for n, g in zip(shape3, nodes3)]
    iz1, iy1, ix1 = np.minimum(iz + 1, nodes3[0] - 1), np.minimum(iy + 1, nodes3[1] - 1), np.minimum(ix + 1, nodes3[2] - 1)
    full = (shape3[0], shape3[1], nodes3[2], 3)
    tzb, tyb = np.broadcast_to(tz[:, None, None, None], full), np.broadcast_to(ty[None, :, None, None], full)
    r0 = io.lerp32(C[iz][:, iy], C[iz1][:, iy], tzb)
    r1 = io.lerp32(C[iz][:, iy1], C[iz1][:, iy1], tzb)
    row = io.lerp32(r0, r1, tyb)
    d = io.lerp32(row[:, :, ix], row[:, :, ix1], np.broadcast_to(tx[None, None, :, None], shape3 + (3,)))
    return d[..., 3 - ndim:].reshape(tuple(shape) + (ndim,))


def warp_float(data, field):
    """I(clamp(p + d(p), 0, n - 1)) in float64: the linear sample of the data (as float32 values) at the clamped coordinates."""
    data = np.asarray(data)
    d = displacement(data.shape, field).astype(np.float64)
    idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in data.shape], indexing="ij")
    coords = np.array([np.clip(idx[ax] + d[..., ax], 0.0, data.shape[ax] - 1.0) for ax in range(data.ndim)])
    return ndimage.map_coordinates(data.astype(np.float32).astype(np.float64), coords, order=1, mode="nearest")


def to_dtype(value, out_dtype):
    """The header's store: float32 as it is; integers rounded half to even, saturated, NaN as 0."""
    out_dtype = np.dtype(out_dtype)
    if out_dtype.kind == "f":
        return value.astype(np.float32)
    r = np.rint(value)
    r = np.where(r >= 0, r, 0.0)
    return np.minimum(r, float(np.iinfo(out_dtype).max)).astype(out_dtype)


def warp(data, field, out_dtype=None):
    return to_dtype(warp_float(data, field), np.asarray(data).dtype if out_dtype is None else out_dtype)
