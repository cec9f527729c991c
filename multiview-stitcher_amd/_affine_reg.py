"""Gauss-Newton intensity registration of two overlap crops (``registration.affine_registration``).

The voxel-sized work of an iteration -- warping the moving crop, the residual and the normal equations -- is one library
call (``mvs_affine_normal_eq``); what stays here is the model algebra on at most 12 parameters, in float64.

``metric="mattes"`` maximises the Mattes mutual information instead (``optimise_mi``): per iteration one joint histogram
(``mvs_affine_joint_hist``) per tried step length and one gradient reduction (``mvs_affine_mi_gradient``); the histogram
algebra -- probabilities, the metric, the table of logarithms -- is B x B float64 work on the host.

Pose convention: ``(A, t)`` is centred and in full-resolution pixels, fixed voxel ``x`` samples moving at
``p = c + t + A (x - c)`` with ``c = (shape - 1) / 2``.  Parameters of the normal equations: the rows of ``[A | t]``.
"""

from __future__ import annotations

import warnings

import numpy as np

MODELS = ("translation", "rigid", "similarity", "affine")
METRICS = ("ssd", "mattes")
MIN_BINS, MAX_BINS = 8, 64
MIN_ALPHA = 2.0 ** -10          # the backtracking search of the mattes loop gives up below this step length (level voxels)


def rotation_generators(ndim):
    """Skew-symmetric generators: one in 2D (y, x), three in 3D ((y, x), (z, x), (z, y))."""
    planes = [(0, 1)] if ndim == 2 else [(1, 2), (0, 2), (0, 1)]
    gens = []
    for i, j in planes:
        g = np.zeros((ndim, ndim))
        g[i, j], g[j, i] = -1.0, 1.0
        gens.append(g)
    return gens


def n_model_params(model, ndim):
    nrot = 1 if ndim == 2 else 3
    return {"translation": ndim, "rigid": ndim + nrot, "similarity": ndim + nrot + 1, "affine": ndim * (ndim + 1)}[model]


def model_jacobian(model, A):
    """B = d theta / d q at the pose: theta the row-major ``[A | t]``, q = (shifts, rotation generators, log scale) or theta."""
    ndim = A.shape[0]
    P = ndim * (ndim + 1)
    if model == "affine":
        return np.eye(P)
    cols = []
    for k in range(ndim):
        d = np.zeros((ndim, ndim + 1))
        d[k, ndim] = 1.0
        cols.append(d.ravel())
    if model in ("rigid", "similarity"):
        gens = rotation_generators(ndim) + ([np.eye(ndim)] if model == "similarity" else [])
        for g in gens:
            d = np.zeros((ndim, ndim + 1))
            d[:, :ndim] = g @ A          # left-multiplicative: dA = G A
            cols.append(d.ravel())
    return np.stack(cols, axis=1)


def exp_generators(w, log_scale, ndim):
    """exp(sum w_m G_m + log_scale I): a rotation (Rodrigues) times exp(log_scale)."""
    if ndim == 2:
        c, s = np.cos(w[0]), np.sin(w[0])
        R = np.array([[c, -s], [s, c]])
    else:
        K = sum(wm * g for wm, g in zip(w, rotation_generators(3)))
        th = float(np.sqrt(np.dot(w, w)))
        if th < 1e-6:
            a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
        else:
            a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
        R = np.eye(3) + a * K + b * (K @ K)
    return np.exp(log_scale) * R


def apply_update(model, A, t, q):
    """The pose after the model step ``q``: additive for translation / affine, ``A <- exp(G) A`` for rigid / similarity."""
    ndim = A.shape[0]
    q = np.asarray(q, dtype=np.float64)
    if model == "affine":
        d = q.reshape(ndim, ndim + 1)
        return A + d[:, :ndim], t + d[:, ndim]
    t = t + q[:ndim]
    if model == "translation":
        return A, t
    nrot = 1 if ndim == 2 else 3
    ls = q[ndim + nrot] if model == "similarity" else 0.0
    return exp_generators(q[ndim:ndim + nrot], ls, ndim) @ A, t


def level_offset(shape, b):
    """d of the level conversion: the binned grid (``n // b`` voxels of b, trimmed at the end) is centred d away from the crop."""
    shape = np.asarray(shape, dtype=np.float64)
    return -(shape - b * np.floor(shape / b)) / 2.0


def to_level(A, t, shape, b):
    return (t + (A - np.eye(len(t))) @ level_offset(shape, b)) / b


def from_level(A, t_b, shape, b):
    return b * t_b - (A - np.eye(len(t_b))) @ level_offset(shape, b)


def corner_displacement(A0, t0, A1, t1, shape):
    """Largest distance between the images of a crop corner under two centred poses (full-resolution px)."""
    half = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    ndim = len(half)
    worst = 0.0
    for bits in range(1 << ndim):
        x = np.array([half[k] if bits >> k & 1 else -half[k] for k in range(ndim)])
        worst = max(worst, float(np.linalg.norm((t1 - t0) + (A1 - A0) @ x)))
    return worst


def pose_to_matrix(A, t, shape):
    ndim = len(t)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    M = np.eye(ndim + 1)
    M[:ndim, :ndim] = A
    M[:ndim, ndim] = c + t - A @ c
    return M


def matrix_to_pose(M, shape):
    M = np.asarray(M, dtype=np.float64)
    ndim = M.shape[0] - 1
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    A = M[:ndim, :ndim].copy()
    return A, M[:ndim, ndim] - c + A @ c


def fit_gain_bias(n, sv, sf, svf, sv2):
    """Least squares F ~ gain v + bias from the moments; None when v has no variance."""
    var = sv2 - sv * sv / n
    if not (n > 1 and var > 0.0):
        return None
    gain = (svf - sv * sf / n) / var
    return gain, (sf - gain * sv) / n


class Refused(Exception):
    pass


def optimise(normal_equations, levels, shape, model, A, t, max_iterations, tolerance, fit_intensity):
    """The coarse-to-fine loop.  ``normal_equations(level_index, A, t_b, gain, bias)`` returns (H, b, sr2, n, moments) of that
    level; ``levels``: the bin of each.  Returns (A, t, history); raises ``Refused`` when a level cannot be solved."""
    ndim = len(shape)
    nq = n_model_params(model, ndim)
    gain, bias = 1.0, 0.0
    history = []
    for li, (b, cap) in enumerate(zip(levels, max_iterations)):
        for _ in range(int(cap)):
            H, g, sr2, n, mom = normal_equations(li, A, to_level(A, t, shape, b), gain, bias)
            if n < 4 * nq:
                raise Refused(f"{int(n)} valid samples for {nq} parameters")
            B = model_jacobian(model, A)
            Hq, gq = B.T @ H @ B, B.T @ g
            try:
                L = np.linalg.cholesky(Hq)
            except np.linalg.LinAlgError:
                raise Refused("the normal equations are not positive definite") from None
            q = -np.linalg.solve(L.T, np.linalg.solve(L, gq))
            A_b, t_b = apply_update(model, A, to_level(A, t, shape, b), q)
            A1, t1 = A_b, from_level(A_b, t_b, shape, b)
            step = corner_displacement(A, t, A1, t1, shape)
            history.append({"level": li, "msd": sr2 / n, "n": int(n), "gain": gain, "bias": bias, "step": step})
            A, t = A1, t1
            if fit_intensity:
                gb = fit_gain_bias(n, *mom[:4])
                if gb is not None:
                    gain, bias = gb
            if step < tolerance:
                break
    return A, t, history


def mutual_information(hist):
    """From a joint histogram (rows: fixed bin, columns: moving bin), in float64: (MI = sum_{P>0} P log(P / (pF pM)), the
    table L = log(P / pM) where P > 0 else 0, the symmetric uncertainty 2 MI / (H_F + H_M))."""
    P = np.asarray(hist, dtype=np.float64)
    P = P / P.sum()
    pF, pM = P.sum(axis=1), P.sum(axis=0)
    pos = P > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        table = np.where(pos, np.log(P / pM[None, :]), 0.0)
        mi = float(np.sum(np.where(pos, P * np.log(P / (pF[:, None] * pM[None, :])), 0.0)))
        entropy = -(np.sum(np.where(pF > 0, pF * np.log(pF), 0.0)) + np.sum(np.where(pM > 0, pM * np.log(pM), 0.0)))
    return mi, table, (2.0 * mi / float(entropy) if entropy > 0 else np.nan)


def bin_ranges(f_lo, f_hi, m_lo, m_hi, n_bins):
    """(f_lo, f_scale, m_lo, m_scale) of the kernels, as float32; raises ``Refused`` when a crop has no spread."""
    if not (f_hi > f_lo and m_hi > m_lo):
        raise Refused("a crop is constant or has no finite value")
    return (np.float32(f_lo), np.float32((n_bins - 1) / (float(f_hi) - float(f_lo))),
            np.float32(m_lo), np.float32((n_bins - 4) / (float(m_hi) - float(m_lo))))


def optimise_mi(metric, gradient, preconditioner, levels, shape, model, A, t, max_iterations, tolerance):
    """The coarse-to-fine loop of ``metric="mattes"`` (ascent).  ``metric(level_index, A, t_b)`` returns (MI, table, n valid) of
    a pose, ``gradient(level_index, A, t_b, table)`` d MI / d theta (theta: the rows of ``[A | t]``) and
    ``preconditioner(level_index, A, t_b)`` the J^T J of the squared-residual metric at gain 1, bias 0; it is taken once per
    level, at the level's first pose.  Per iteration: the direction ``(B^T H B)^-1 B^T g`` scaled to one level voxel of corner
    displacement, then a backtracking search on the step length alpha, from ``min(1, 2 * previous alpha)`` down to
    ``MIN_ALPHA``, for a pose of larger MI (one ``metric`` call per trial).  A level ends when no alpha is found, when the
    accepted step moves no corner by ``tolerance`` or at its cap.  Returns (A, t, history)."""
    ndim = len(shape)
    nq = n_model_params(model, ndim)
    history = []
    for li, (b, cap) in enumerate(zip(levels, max_iterations)):
        t_b = to_level(A, t, shape, b)
        mi, table, n = metric(li, A, t_b)
        if n < 4 * nq:
            raise Refused(f"{int(n)} valid samples for {nq} parameters")
        H = preconditioner(li, A, t_b)
        alpha = 0.5
        for _ in range(int(cap)):
            t_b = to_level(A, t, shape, b)
            g = gradient(li, A, t_b, table)
            B = model_jacobian(model, A)
            try:
                L = np.linalg.cholesky(B.T @ H @ B)
            except np.linalg.LinAlgError:
                raise Refused("the preconditioner is not positive definite") from None
            s = np.linalg.solve(L.T, np.linalg.solve(L, B.T @ g))

            def moved(q):
                A1, t1_b = apply_update(model, A, t_b, q)
                return A1, from_level(A1, t1_b, shape, b)

            d1 = corner_displacement(A, t, *moved(s), shape)
            if not (d1 > 0.0 and np.isfinite(d1)):
                break
            s = s * (b / d1)
            alpha = min(1.0, 2.0 * alpha)
            found = None
            while alpha >= MIN_ALPHA:
                A1, t1 = moved(alpha * s)
                trial = metric(li, A1, to_level(A1, t1, shape, b))
                if trial[2] >= 4 * nq and trial[0] > mi:
                    found = trial
                    break
                alpha /= 2.0
            if found is None:
                history.append({"level": li, "mi": mi, "n": int(n), "alpha": 0.0, "step": 0.0})
                break
            step = corner_displacement(A, t, A1, t1, shape)
            history.append({"level": li, "mi": mi, "n": int(n), "alpha": alpha, "step": step})
            A, t = A1, t1
            mi, table, n = found
            if step < tolerance:
                break
    return A, t, history


def affine_registration(fixed_data, moving_data, transform_type="rigid", shrink_factors=(2, 1), max_iterations=(30, 20), tolerance=1e-3,
                        initial_affine="phase_correlation", fit_intensity=True, device=0, return_debug=False, metric="ssd", n_bins=32):
    """See ``registration.affine_registration``."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}")
    if not (isinstance(n_bins, (int, np.integer)) and MIN_BINS <= n_bins <= MAX_BINS):
        raise ValueError(f"n_bins must be an integer in {MIN_BINS}..{MAX_BINS}")
    if transform_type not in MODELS:
        raise ValueError(f"transform_type must be one of {MODELS}")

    from . import _reg_ops, registration
    from .device import DeviceArray, is_device_array
    from .transformation import resample_array

    if len(shrink_factors) != len(max_iterations):
        raise ValueError("shrink_factors and max_iterations must have the same length")
    F = registration._as_array(fixed_data)
    M = registration._as_array(moving_data)
    if tuple(F.shape) != tuple(M.shape):
        raise ValueError("fixed and moving crops must have the same shape")
    shape = tuple(int(s) for s in F.shape)
    ndim = len(shape)
    if ndim not in (2, 3):
        raise ValueError("crops must be 2D or 3D")
    if not is_device_array(F):
        # host crops are uploaded once: every iteration reads both, and so do the initial pose and the quality
        F = DeviceArray.from_host(np.ascontiguousarray(F, dtype=np.float32), device)
        M = DeviceArray.from_host(np.ascontiguousarray(M, dtype=np.float32), device)

    if isinstance(initial_affine, str):
        if initial_affine not in ("phase_correlation", "identity"):
            raise ValueError("initial_affine must be 'phase_correlation', 'identity' or a matrix")
        M0 = np.eye(ndim + 1)
        if initial_affine == "phase_correlation":
            try:
                res = registration.phase_correlation_registration(F, M, device=device)
                if isinstance(res, dict):
                    M0 = np.asarray(res["affine_matrix"], dtype=np.float64)
            except ValueError:
                pass
    else:
        M0 = np.asarray(initial_affine, dtype=np.float64)
        if M0.shape != (ndim + 1, ndim + 1):
            raise ValueError("initial_affine must be an (ndim + 1) x (ndim + 1) matrix")
    A0, t0 = matrix_to_pose(M0, shape)

    def result(A, t, quality, history):
        out = {"affine_matrix": pose_to_matrix(A, t, shape), "quality": quality}
        if return_debug:
            out["debug"] = {"history": history, "initial_affine": pose_to_matrix(A0, t0, shape)}
        return out

    levels, crops, caps = [], [], []
    for b, cap in zip(shrink_factors, max_iterations):
        b = int(b)
        if b < 1:
            raise ValueError("shrink factors must be positive")
        if b == 1:
            crops.append((F, M))
        elif min(s // b for s in shape) < 4:
            continue                     # nothing left of the crop at this bin
        else:
            crops.append((_reg_ops.bin_mean(F, [b] * ndim, device), _reg_ops.bin_mean(M, [b] * ndim, device)))
        levels.append(b)
        caps.append(int(cap))

    def normal_equations(li, A, t_b, gain, bias):
        return _reg_ops.affine_normal_equations(crops[li][0], crops[li][1], A, t_b, gain, bias, device)

    n_bins = int(n_bins)
    ranges = {}

    def level_ranges(F_l, M_l):
        f_lo, f_hi, _ = _reg_ops.finite_range(F_l, device)
        m_lo, m_hi, _ = _reg_ops.finite_range(M_l, device)
        return bin_ranges(f_lo, f_hi, m_lo, m_hi, n_bins)

    def mi_metric(li, A, t_b):
        if li not in ranges:
            ranges[li] = level_ranges(*crops[li])
        hist, n = _reg_ops.affine_joint_hist(crops[li][0], crops[li][1], A, t_b, n_bins, ranges[li], device)
        if n == 0:
            return -np.inf, None, 0
        mi, table, _ = mutual_information(hist)
        return mi, table, n

    def mi_gradient(li, A, t_b, table):
        sums, n = _reg_ops.affine_mi_gradient(crops[li][0], crops[li][1], A, t_b, n_bins, ranges[li], table, device)
        return (float(ranges[li][3]) / n) * sums

    try:
        if metric == "mattes":
            A, t, history = optimise_mi(mi_metric, mi_gradient, lambda li, A, t_b: normal_equations(li, A, t_b, 1.0, 0.0)[0], levels,
                                        shape, transform_type, A0, t0, caps, tolerance)
            # quality: the symmetric uncertainty 2 MI / (H_F + H_M) of the full-resolution histogram at the result, in [0, 1]
            # (a rank correlation means nothing across a relation that is not monotone)
            hist, n = _reg_ops.affine_joint_hist(F, M, A, t, n_bins, level_ranges(F, M), device)
            return result(A, t, mutual_information(hist)[2] if n > 0 else np.nan, history)
        A, t, history = optimise(normal_equations, levels, shape, transform_type, A0, t0, caps, tolerance, fit_intensity)
    except Refused as e:
        warnings.warn(f"affine_registration: {e}; returning the initial pose.", UserWarning, stacklevel=3)
        return result(A0, t0, np.nan, [])

    # quality as phase_correlation_registration reports it: masked Spearman coefficient of the rescaled crops, moving resampled by the result
    Fr = _reg_ops.rescale_intensity(F, device, out_on_device=True)[0]
    Mr = _reg_ops.rescale_intensity(M, device, out_on_device=True)[0]
    Mfinal = pose_to_matrix(A, t, shape)
    Mw = resample_array(Mr, Mfinal[:ndim, :ndim], Mfinal[:ndim, ndim], shape, order=1, cval=np.nan, device=device)
    # ("intersection": the warp leaves NaN outside the moving crop)
    _, spear, code = _reg_ops.score_candidates(Fr, Mw, [[0.0] * ndim], "intersection", 1.0, 0.0, device, quality_for_all=True)
    quality = float(spear[0]) if code[0] == 0 else np.nan
    return result(A, t, quality, history)
