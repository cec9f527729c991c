"""Plain numpy restatement of the Mattes mutual-information metric of affine_registration (csrc/mvs_affine_mi_dev.h,
mvs_affine_joint_hist, mvs_affine_mi_gradient, the ``mattes`` loop of _affine_reg.py), written from the specification and
independent of the package.  Warp, validity and model algebra come from tests/affine_reg_oracle.py.

Two modes.  ``np.float32``: the per-sample quantities follow the header operation by operation in float32 (numpy rounds every
elementwise operation on its own, like a build with -ffp-contract=off), the histogram weights are the header's integers and
the table is float32; only the sums are float64.  ``np.float64``: everything in float64 with the window's real-valued weights --
a differentiable function of the pose, the yardstick of the gradient.
"""
import numpy as np

from tests import affine_reg_oracle as ao

WEIGHT_ONE = 1048576.0      # 2^20


# ---- per-sample arithmetic --------------------------------------------------------------------------------------------
def beta3(t, dt=np.float32):
    """Cubic B-spline, explicit products and sums in ``dt``."""
    dt = np.dtype(dt).type
    t = np.asarray(t, dtype=dt)
    a = np.abs(t)
    inner = dt(2.0 / 3.0) + (a * a) * (dt(0.5) * a - dt(1.0))
    d = dt(2.0) - a
    outer = ((d * d) * d) * dt(1.0 / 6.0)
    return np.where(a < 1, inner, np.where(a < 2, outer, dt(0.0))).astype(dt)


def beta3_prime(t, dt=np.float32):
    dt = np.dtype(dt).type
    t = np.asarray(t, dtype=dt)
    a = np.abs(t)
    inner = t * (dt(1.5) * a - dt(2.0))
    d = dt(2.0) - a
    outer = np.where(t < 0, dt(0.5), dt(-0.5)).astype(dt) * (d * d)
    return np.where(a < 1, inner, np.where(a < 2, outer, dt(0.0))).astype(dt)


def fixed_bin(F, f_lo, f_scale, B, dt=np.float32):
    dt = np.dtype(dt).type
    r = np.floor((np.asarray(F, dtype=dt) - dt(f_lo)) * dt(f_scale) + dt(0.5))
    return np.clip(r, 0, B - 1).astype(np.int64)


def moving_coord(v, m_lo, m_scale, B, dt=np.float32):
    dt = np.dtype(dt).type
    u = (np.asarray(v, dtype=dt) - dt(m_lo)) * dt(m_scale) + dt(1.5)
    return np.minimum(np.maximum(u, dt(1.5)), dt(B - 2.5)).astype(dt)


def window(u, dt=np.float32):
    """(first tap b_0, the four arguments u - b_k as a (4, n) array)."""
    dt = np.dtype(dt).type
    b0 = np.floor(u).astype(np.int64) - 1
    return b0, np.stack([u - (b0 + k).astype(dt) for k in range(4)])


def quantise(w):
    """Integer histogram weight of a float32 window value."""
    return (np.asarray(w, dtype=np.float32) * np.float32(WEIGHT_ONE) + np.float32(0.5)).astype(np.int64)


def finite_range(a):
    a = np.asarray(a)
    a = a[np.isfinite(a)]
    return (float(a.min()), float(a.max())) if a.size else (np.nan, np.nan)


def ranges(F, M, B):
    """(f_lo, f_scale, m_lo, m_scale) as the host passes them: computed in float64, rounded to float32.  None when a crop has no
    finite value or only one."""
    f_lo, f_hi = finite_range(F)
    m_lo, m_hi = finite_range(M)
    if not (f_hi > f_lo and m_hi > m_lo):
        return None
    return np.float32(f_lo), np.float32((B - 1) / (f_hi - f_lo)), np.float32(m_lo), np.float32((B - 4) / (m_hi - m_lo))


# ---- histogram, metric, gradient ------------------------------------------------------------------------------------------
def _binned_samples(F, M, A, t, B, rng, dt):
    valid, v, g, _, Fd, d = ao.samples(F, M, A, t, 1.0, 0.0, dt)
    a = fixed_bin(Fd[valid], rng[0], rng[1], B, dt)
    u = moving_coord(v[valid], rng[2], rng[3], B, dt)
    b0, args = window(u, dt)
    return valid, a, b0, args, [gk[valid] for gk in g], d


def joint_hist(F, M, A, t, B, rng, sample_dtype=np.float32):
    """(hist (B, B), n_valid): int64 sums of the quantised weights in float32 mode, float64 sums of the weights in float64 mode."""
    dt = np.dtype(sample_dtype).type
    valid, a, b0, args, _, _ = _binned_samples(F, M, A, t, B, rng, dt)
    exact = dt is np.float32
    hist = np.zeros((B, B), dtype=np.int64 if exact else np.float64)
    for k in range(4):
        w = beta3(args[k], dt)
        np.add.at(hist, (a, b0 + k), quantise(w) if exact else w)
    return hist, int(valid.sum())


def mutual_information(hist):
    """(MI, table L = log(P / pM) where P > 0 else 0, symmetric uncertainty 2 MI / (H_F + H_M)); float64."""
    P = hist.astype(np.float64) / float(hist.sum())
    pF, pM = P.sum(axis=1), P.sum(axis=0)
    pos = P > 0
    outer = np.where(pos, pF[:, None] * pM[None, :], 1.0)
    Ps = np.where(pos, P, 1.0)
    mi = float(np.sum(np.where(pos, P * np.log(Ps / outer), 0.0)))
    table = np.where(pos, np.log(Ps / np.where(pos, np.broadcast_to(pM, P.shape), 1.0)), 0.0)
    ent = lambda p: -float(np.sum(p[p > 0] * np.log(p[p > 0])))   # noqa: E731
    denom = ent(pF) + ent(pM)
    return mi, table, (2.0 * mi / denom if denom > 0 else np.nan)


def gradient_samples(F, M, A, t, B, rng, table, sample_dtype=np.float32):
    """Per valid sample: (w, [g_k], [(x - c)_m ..., 1]); w and g in ``sample_dtype``, the coordinates float64."""
    dt = np.dtype(sample_dtype).type
    valid, a, b0, args, g, d = _binned_samples(F, M, A, t, B, rng, dt)
    tab = np.asarray(table, dtype=dt)
    w = beta3_prime(args[0], dt) * tab[a, b0]
    for k in range(1, 4):
        w = w + beta3_prime(args[k], dt) * tab[a, b0 + k]
    return w, g, [np.broadcast_to(dk, valid.shape)[valid] for dk in d] + [np.ones(a.size)]


def gradient_sums(F, M, A, t, B, rng, table, sample_dtype=np.float32):
    """(out (P,), n_valid): out[k (nd + 1) + m] = sum w g_k (x - c)_m, m = nd: sum w g_k.  w and w g_k in ``sample_dtype``, the
    sums in float64."""
    w, g, xt = gradient_samples(F, M, A, t, B, rng, table, sample_dtype)
    nd = len(g)
    out = np.array([float(np.sum((w * g[k]).astype(np.float64) * xt[m])) for k in range(nd) for m in range(nd + 1)])
    return out, w.size


def metric(F, M, A, t, B, rng, sample_dtype=np.float32):
    """(MI, table in the mode's dtype, n_valid, symmetric uncertainty)."""
    hist, n = joint_hist(F, M, A, t, B, rng, sample_dtype)
    if n == 0:
        return -np.inf, None, 0, np.nan
    mi, table, su = mutual_information(hist)
    return mi, table.astype(sample_dtype), n, su


def gradient(F, M, A, t, B, rng, table, sample_dtype=np.float32):
    """d MI / d theta, theta the rows of [A | t]: (m_scale / n_valid) * the sums."""
    out, n = gradient_sums(F, M, A, t, B, rng, table, sample_dtype)
    return (float(rng[3]) / n) * out


# ---- the loop -------------------------------------------------------------------------------------------------------------
MIN_ALPHA = 2.0 ** -10


def register(F, M, transform_type="rigid", shrink_factors=(2, 1), max_iterations=(30, 20), tolerance=1e-3, initial_affine="identity",
             n_bins=32, sample_dtype=np.float32):
    """The ``mattes`` loop of affine_registration.  Per level: the preconditioner H (J^T J of the squared-residual metric at gain
    1, bias 0) once at the level's first pose; per iteration the gradient at the current pose, the direction
    (B^T H B)^-1 B^T g scaled to one level voxel of corner displacement, and a backtracking search on the step length.  Returns
    {"affine_matrix", "A", "t", "history", "quality"}; raises ao.Refused where the function under test warns."""
    shape, nd = F.shape, F.ndim
    m0 = np.eye(nd + 1) if isinstance(initial_affine, str) else initial_affine
    A, t = ao.matrix_to_pose(m0, shape)
    nq = ao.n_params(transform_type, nd)
    history, level = [], -1
    for b, cap in zip(shrink_factors, max_iterations):
        if b > 1 and min(n // b for n in shape) < 4:
            continue
        level += 1
        Fb, Mb = ao.bin_mean(F, b), ao.bin_mean(M, b)
        rng = ranges(Fb, Mb, n_bins)
        if rng is None:
            raise ao.Refused("a crop is constant")
        tb = ao.to_level(A, t, shape, b)
        mi, table, n, _ = metric(Fb, Mb, A, tb, n_bins, rng, sample_dtype)
        if n < 4 * nq:
            raise ao.Refused("too few valid samples")
        H = ao.normal_equations(Fb, Mb, A, tb, 1.0, 0.0, sample_dtype)[0]
        alpha = 0.5
        for _ in range(cap):
            tb = ao.to_level(A, t, shape, b)
            g = gradient(Fb, Mb, A, tb, n_bins, rng, table, sample_dtype)
            Bm = ao.jacobian(transform_type, A)
            Hq = Bm.T @ H @ Bm
            if np.linalg.eigvalsh(Hq).min() <= 0.0:
                raise ao.Refused("not positive definite")
            s = np.linalg.solve(Hq, Bm.T @ g)

            def moved(q):
                A1, tb1 = ao.update(transform_type, A, tb, q)
                return A1, ao.from_level(A1, tb1, shape, b)

            d1 = ao.corner_displacement(A, t, *moved(s), shape)
            if not (d1 > 0.0 and np.isfinite(d1)):
                break
            s = s * (b / d1)
            alpha = min(1.0, 2.0 * alpha)
            found = None
            while alpha >= MIN_ALPHA:
                A1, t1 = moved(alpha * s)
                trial = metric(Fb, Mb, A1, ao.to_level(A1, t1, shape, b), n_bins, rng, sample_dtype)
                if trial[2] >= 4 * nq and trial[0] > mi:
                    found = trial
                    break
                alpha /= 2.0
            if found is None:
                history.append({"level": level, "mi": mi, "n": n, "alpha": 0.0, "step": 0.0})
                break
            step = ao.corner_displacement(A, t, A1, t1, shape)
            history.append({"level": level, "mi": mi, "n": n, "alpha": alpha, "step": step})
            A, t = A1, t1
            mi, table, n, _ = found
            if step < tolerance:
                break
    rng = ranges(F, M, n_bins)
    quality = metric(F, M, A, t, n_bins, rng, sample_dtype)[3] if rng is not None else np.nan
    return {"affine_matrix": ao.pose_to_matrix(A, t, shape), "A": A, "t": t, "history": history, "quality": quality}


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------
def remap(v):
    """The intensity relation no gain and offset can describe: |2 v - 2 median(v)| (NaN stays NaN)."""
    v = np.asarray(v, dtype=np.float64)
    return np.abs(2.0 * v - 2.0 * np.nanmedian(v)).astype(np.float32)


def make_pair(shape, seed, model, sigma=3.0, t0=None, A0=None):
    """(F, M, A0, t0): F the central crop of smooth noise (Gaussian ``sigma``), M the same scene seen through the inverse of the
    pose (A0, t0) (order 3) and remapped by ``remap``.  (A0, t0) is what a registration should return."""
    from scipy import ndimage

    nd = len(shape)
    pad = 12
    rng = np.random.default_rng(seed)
    G = ndimage.gaussian_filter(rng.random(tuple(n + 2 * pad for n in shape)), sigma)
    G = (G - G.min()) / (G.max() - G.min())
    F = np.ascontiguousarray(G[tuple(slice(pad, pad + n) for n in shape)], dtype=np.float32)
    if A0 is None:
        A0, t0 = ao.true_pose(model, nd, seed, t0)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    R = np.linalg.inv(A0)
    s = -R @ t0
    Mv = ndimage.affine_transform(G, R, offset=pad + c + s - R @ c, output_shape=shape, order=3, mode="nearest")
    return F, np.ascontiguousarray(remap(Mv)), A0, np.asarray(t0, dtype=np.float64)
