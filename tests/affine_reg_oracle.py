"""Plain numpy restatement of the Gauss-Newton intensity registration (csrc/mvs_affine_reg_dev.h, _affine_reg.py), written
from the specification and independent of the package.

``normal_equations(..., sample_dtype=np.float64)`` is the yardstick; with ``np.float32`` the per-sample quantities (fraction,
interpolated value, gradient, residual) follow the header operation by operation in float32 -- numpy rounds every elementwise
operation on its own, like a build with -ffp-contract=off -- and only the sums are float64.

Pose: centred, ``p = c + t + A (x - c)`` with ``c = (shape - 1) / 2``; parameters are the rows of ``[A | t]``.
"""
import numpy as np
from scipy import linalg, ndimage

MODELS = ("translation", "rigid", "similarity", "affine")


# ---- per-sample arithmetic --------------------------------------------------------------------------------------------
def coord(a_row, d, o):
    """One coordinate in the header's order: ((a_0 d_0 + a_1 d_1) + a_2 d_2) + o, every operation rounded on its own."""
    acc = a_row[0] * d[0] + a_row[1] * d[1]
    if len(d) == 3:
        acc = acc + a_row[2] * d[2]
    return acc + o


def coordinates(shape, A, t):
    """p_k on the whole grid, in the header's order: ((A_k0 d_0 + A_k1 d_1) + A_k2 d_2) + (c_k + t_k)."""
    nd = len(shape)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    d = np.meshgrid(*[np.arange(n, dtype=np.float64) - ck for n, ck in zip(shape, c)], indexing="ij", sparse=True)
    A = np.asarray(A, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    return [np.broadcast_to(coord(A[k], d, c[k] + t[k]), shape) for k in range(nd)], d


def split(p, n, dtype):
    """(inside, i0, fraction): inside iff i0 >= 0 and i0 + 1 <= n - 1."""
    with np.errstate(invalid="ignore"):
        inside = (p >= 0.0) & (p < float(n - 1))
    fl = np.floor(np.where(inside, p, 0.0))
    return inside, fl.astype(np.int64), (np.where(inside, p, 0.0) - fl).astype(dtype)


def sample(taps, fr):
    """Value and gradient of the bi / trilinear interpolant.  taps[(bz,) by, bx], fr = fractions (z,) y, x; one dtype throughout."""
    if len(fr) == 2:
        fy, fx = fr
        dx0, dx1 = taps[0, 1] - taps[0, 0], taps[1, 1] - taps[1, 0]
        c0, c1 = taps[0, 0] + fx * dx0, taps[1, 0] + fx * dx1
        dy = c1 - c0
        return c0 + fy * dy, [dy, dx0 + fy * (dx1 - dx0)]
    fz, fy, fx = fr
    dx00, dx01 = taps[0, 0, 1] - taps[0, 0, 0], taps[0, 1, 1] - taps[0, 1, 0]
    dx10, dx11 = taps[1, 0, 1] - taps[1, 0, 0], taps[1, 1, 1] - taps[1, 1, 0]
    c00, c01 = taps[0, 0, 0] + fx * dx00, taps[0, 1, 0] + fx * dx01
    c10, c11 = taps[1, 0, 0] + fx * dx10, taps[1, 1, 0] + fx * dx11
    dy0, dy1 = c01 - c00, c11 - c10
    c0, c1 = c00 + fy * dy0, c10 + fy * dy1
    dz = c1 - c0
    e0, e1 = dx00 + fy * (dx01 - dx00), dx10 + fy * (dx11 - dx10)
    return c0 + fz * dz, [dz, dy0 + fz * (dy1 - dy0), e0 + fz * (e1 - e0)]


def samples(F, M, A, t, gain=1.0, bias=0.0, sample_dtype=np.float64):
    """Per voxel: valid, v, g (list), r -- in ``sample_dtype`` -- and the centred coordinates d (float64, sparse)."""
    F = np.asarray(F, dtype=np.float32)
    M = np.asarray(M, dtype=np.float32)
    shape, nd, dt = F.shape, F.ndim, np.dtype(sample_dtype).type
    p, d = coordinates(shape, A, t)
    valid = np.isfinite(F)
    i0, fr = [], []
    for k in range(nd):
        ins, i, f = split(p[k], shape[k], dt)
        valid = valid & ins
        i0.append(i)
        fr.append(f)
    taps = np.empty((2,) * nd + shape, dtype=dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for bits in np.ndindex(*(2,) * nd):
            tap = M[tuple(np.where(valid, i + b, 0) for i, b in zip(i0, bits))].astype(dt)
            valid = valid & np.isfinite(tap)
            taps[bits] = tap
        taps[..., ~valid] = 0
        v, g = sample(taps, fr)
        Fd = np.where(valid, F, 0).astype(dt)
        r = (dt(gain) * v + dt(bias)) - Fd
    return valid, v, g, r, Fd, d


def normal_equations(F, M, A, t, gain=1.0, bias=0.0, sample_dtype=np.float64):
    """(H (P, P), b (P,), sum r^2, n, (sum v, sum F, sum vF, sum v^2, sum F^2)); sums in float64."""
    dt = np.dtype(sample_dtype).type
    valid, v, g, r, Fd, d = samples(F, M, A, t, gain, bias, sample_dtype)
    nd = len(g)
    shape = valid.shape
    xt = [np.broadcast_to(dk, shape)[valid] for dk in d] + [np.ones(int(valid.sum()))]
    gg = [(dt(gain) * gk)[valid].astype(np.float64) for gk in g]
    J = np.stack([gg[k] * xt[j] for k in range(nd) for j in range(nd + 1)], axis=1)
    r64 = r[valid].astype(np.float64)
    v64, F64 = v[valid].astype(np.float64), Fd[valid].astype(np.float64)
    mom = (v64.sum(), F64.sum(), (v64 * F64).sum(), (v64 * v64).sum(), (F64 * F64).sum())
    return J.T @ J, J.T @ r64, float(r64 @ r64), int(valid.sum()), tuple(float(m) for m in mom)


# ---- model algebra ------------------------------------------------------------------------------------------------------
def generators(nd):
    planes = [(0, 1)] if nd == 2 else [(1, 2), (0, 2), (0, 1)]
    out = []
    for i, j in planes:
        g = np.zeros((nd, nd))
        g[i, j], g[j, i] = -1.0, 1.0
        out.append(g)
    return out


def n_params(model, nd):
    nrot = len(generators(nd))
    return {"translation": nd, "rigid": nd + nrot, "similarity": nd + nrot + 1, "affine": nd * (nd + 1)}[model]


def update(model, A, t, q):
    nd = len(t)
    if model == "affine":
        dq = np.asarray(q).reshape(nd, nd + 1)
        return A + dq[:, :nd], t + dq[:, nd]
    t = t + q[:nd]
    if model == "translation":
        return A, t
    gens = generators(nd) + ([np.eye(nd)] if model == "similarity" else [])
    return linalg.expm(sum(qk * g for qk, g in zip(q[nd:], gens))) @ A, t


def jacobian(model, A):
    """d theta / d q at q = 0 by construction (columns: one unit step of each model parameter, linearised)."""
    nd = A.shape[0]
    if model == "affine":
        return np.eye(nd * (nd + 1))
    cols = []
    for k in range(nd):
        e = np.zeros((nd, nd + 1))
        e[k, nd] = 1.0
        cols.append(e.ravel())
    if model != "translation":
        for g in generators(nd) + ([np.eye(nd)] if model == "similarity" else []):
            e = np.zeros((nd, nd + 1))
            e[:, :nd] = g @ A
            cols.append(e.ravel())
    return np.stack(cols, axis=1)


def level_d(shape, b):
    shape = np.asarray(shape)
    return -(shape - b * (shape // b)) / 2.0


def to_level(A, t, shape, b):
    return (t + (A - np.eye(len(t))) @ level_d(shape, b)) / b


def from_level(A, tb, shape, b):
    return b * tb - (A - np.eye(len(tb))) @ level_d(shape, b)


def bin_mean(a, b):
    """coarsen(b, boundary="trim").mean() in float64, back to float32: a NaN contributor makes the voxel NaN."""
    if b == 1:
        return np.asarray(a, dtype=np.float32)
    nb = [n // b for n in a.shape]
    a = a[tuple(slice(0, n * b) for n in nb)].astype(np.float64)
    a = a.reshape([v for n in nb for v in (n, b)])
    return a.mean(axis=tuple(range(1, 2 * len(nb), 2))).astype(np.float32)


def corner_displacement(A0, t0, A1, t1, shape):
    half = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    worst = 0.0
    for signs in np.ndindex(*(2,) * len(half)):
        x = half * (2.0 * np.asarray(signs) - 1.0)
        worst = max(worst, float(np.linalg.norm((t1 - t0) + (A1 - A0) @ x)))
    return worst


def pose_to_matrix(A, t, shape):
    nd = len(t)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    m = np.eye(nd + 1)
    m[:nd, :nd] = A
    m[:nd, nd] = c + t - A @ c
    return m


def matrix_to_pose(m, shape):
    m = np.asarray(m, dtype=np.float64)
    nd = m.shape[0] - 1
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    return m[:nd, :nd].copy(), m[:nd, nd] - c + m[:nd, :nd] @ c


class Refused(Exception):
    pass


def register(F, M, transform_type="rigid", shrink_factors=(2, 1), max_iterations=(30, 20), tolerance=1e-3, initial_affine="identity",
             fit_intensity=True, sample_dtype=np.float64):
    """The loop of affine_registration.  Returns {"affine_matrix", "A", "t", "history"}; raises Refused where the function
    under test warns and returns its initial pose."""
    shape, nd = F.shape, F.ndim
    m0 = np.eye(nd + 1) if isinstance(initial_affine, str) else initial_affine
    A, t = matrix_to_pose(m0, shape)
    nq = n_params(transform_type, nd)
    gain, bias, history = 1.0, 0.0, []
    level = -1
    for b, cap in zip(shrink_factors, max_iterations):
        if b > 1 and min(n // b for n in shape) < 4:
            continue
        level += 1
        Fb, Mb = bin_mean(F, b), bin_mean(M, b)
        for _ in range(cap):
            tb = to_level(A, t, shape, b)
            H, g, sr2, n, mom = normal_equations(Fb, Mb, A, tb, gain, bias, sample_dtype)
            if n < 4 * nq:
                raise Refused("too few valid samples")
            B = jacobian(transform_type, A)
            Hq = B.T @ H @ B
            if np.linalg.eigvalsh(Hq).min() <= 0.0:
                raise Refused("not positive definite")
            q = -np.linalg.solve(Hq, B.T @ g)
            A1, tb1 = update(transform_type, A, tb, q)
            t1 = from_level(A1, tb1, shape, b)
            step = corner_displacement(A, t, A1, t1, shape)
            history.append({"level": level, "msd": sr2 / n, "n": n, "gain": gain, "bias": bias, "step": step})
            A, t = A1, t1
            if fit_intensity:
                sv, sf, svf, sv2, _ = mom
                var = sv2 - sv * sv / n
                if var > 0.0:
                    gain = (svf - sv * sf / n) / var
                    bias = (sf - gain * sv) / n
            if step < tolerance:
                break
    return {"affine_matrix": pose_to_matrix(A, t, shape), "A": A, "t": t, "history": history}


# ---- the inputs the tests share ---------------------------------------------------------------------------------------------
def true_pose(model, nd, seed, t0=None):
    """The known map: 2 deg in (y, x), in 3D also -1.2 deg in (z, x); scale 1.02 for similarity; a seeded shear on top for affine."""
    t0 = np.asarray((1.3, -0.8, 0.6)[3 - nd:] if t0 is None else t0, dtype=np.float64)
    A = np.eye(nd)
    if model != "translation":
        a = np.deg2rad(2.0)
        R = np.eye(nd)
        R[nd - 2:, nd - 2:] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        if nd == 3:
            b = np.deg2rad(-1.2)
            R = R @ np.array([[np.cos(b), 0, -np.sin(b)], [0, 1, 0], [np.sin(b), 0, np.cos(b)]])
        A = R
        if model == "similarity":
            A = 1.02 * A
        if model == "affine":
            A = A @ (np.eye(nd) + 0.02 * np.random.default_rng(seed + 1000).standard_normal((nd, nd)))
    return A, t0


def make_pair(shape, seed, model, t0=None):
    """(F, M, A0, t0): F the central crop of a smooth ground truth, M the ground truth seen through the inverse of the pose
    (A0, t0) (order 3), times 1.1 plus 0.05, its first three x columns NaN.  (A0, t0) is what a registration should return."""
    nd = len(shape)
    pad = 12
    rng = np.random.default_rng(seed)
    G = ndimage.gaussian_filter(rng.random(tuple(n + 2 * pad for n in shape)), 2.0)
    G = (G - G.min()) / (G.max() - G.min())
    F = np.ascontiguousarray(G[tuple(slice(pad, pad + n) for n in shape)], dtype=np.float32)
    A0, t0 = true_pose(model, nd, seed, t0)
    c = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    R = np.linalg.inv(A0)                       # M[y] = G(pad + c + R (y - c) + s), s = -R t0
    s = -R @ t0
    Mv = ndimage.affine_transform(G, R, offset=pad + c + s - R @ c, output_shape=shape, order=3, mode="nearest")
    Mv = (1.1 * Mv + 0.05).astype(np.float32)
    Mv[..., :3] = np.nan
    return F, np.ascontiguousarray(Mv), A0, t0
