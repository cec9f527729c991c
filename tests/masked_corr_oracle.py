"""numpy-only oracle of registration.masked_correlation_registration (mvs_masked_corr): the definition as a float64 brute-force sum over
every shift of the window (or over a list of shifts), the same definition through float64 transforms for windows too large for the
sum, and a float32 restatement of the device chain (statistics, pack, transforms, spectral combine, window
search) that sizes the tolerances of the GPU tests on the CPU."""
import itertools

import numpy as np

FLT_EPS = float(np.finfo(np.float32).eps)
STATUS_OK, STATUS_NO_ELIGIBLE_SHIFT, STATUS_TOO_FEW_VALID, STATUS_CONSTANT_CROP = 0, 1, 2, 3


def validity(im, mask=None, valid_above=None):
    v = np.isfinite(im)
    if mask is not None:
        v &= np.asarray(mask) != 0
    if valid_above is not None:
        with np.errstate(invalid="ignore"):
            v &= im.astype(np.float64) > float(valid_above)
    return v


def default_shifts(shape, max_shift=None):
    if max_shift is None:
        return [n - 1 for n in shape]
    vals = [max_shift] * len(shape) if np.isscalar(max_shift) else list(max_shift)
    return [min(int(v), n - 1) for v, n in zip(vals, shape)]


def padded_shape(shape, shifts):
    return tuple(1 if n == 1 else 1 << int(n + s - 1).bit_length() for n, s in zip(shape, shifts))


def select(F, M, vF, vM, r, n, den_ok, overlap_ratio, min_overlap):
    """Eligibility, arg-max (lowest flat index among equals) and status from the window volumes."""
    n_max = int(n.max())
    eligible = n >= max(overlap_ratio * n_max, min_overlap)
    if vF.sum() < min_overlap or vM.sum() < min_overlap:
        status = STATUS_TOO_FEW_VALID
    elif F[vF].min() == F[vF].max() or M[vM].min() == M[vM].max():
        status = STATUS_CONSTANT_CROP
    elif not (eligible & den_ok).any():
        status = STATUS_NO_ELIGIBLE_SHIFT
    else:
        status = STATUS_OK
    peak_w = np.unravel_index(int(np.argmax(np.where(eligible, r, -np.inf))), r.shape) if eligible.any() else None
    return eligible, n_max, peak_w, status


def brute_force_at(F, M, shifts, fixed_mask=None, moving_mask=None, valid_above=(None, None)):
    """The definition at the given shifts (a sequence of ndim-tuples), in float64: the overlap count ``n``, the numerator ``num`` and
    the denominator ``den`` of Pearson's r over the voxels valid in both crops, one entry per shift (0 where nothing overlaps)."""
    shape = F.shape
    vF, vM = validity(F, fixed_mask, valid_above[0]), validity(M, moving_mask, valid_above[1])
    shifts = [tuple(int(k) for k in s) for s in shifts]
    num, den, n = np.zeros(len(shifts)), np.zeros(len(shifts)), np.zeros(len(shifts), dtype=np.int64)
    F64, M64 = np.where(vF, F, 0).astype(np.float64), np.where(vM, M, 0).astype(np.float64)
    for w, s in enumerate(shifts):
        slF = tuple(slice(max(0, -k), min(m, m - k)) for k, m in zip(s, shape))      # x
        slM = tuple(slice(max(0, k), min(m, m + k)) for k, m in zip(s, shape))       # x + s
        both = vF[slF] & vM[slM]
        n[w] = both.sum()
        if n[w] == 0:
            continue
        a, b = F64[slF][both], M64[slM][both]
        a, b = a - a.mean(), b - b.mean()
        num[w] = (a * b).sum()
        den[w] = np.sqrt((a * a).sum() * (b * b).sum())
    return n, num, den


def brute_force(F, M, fixed_mask=None, moving_mask=None, valid_above=(None, None), overlap_ratio=0.3, min_overlap=None, max_shift=None):
    """The definition, in float64.  Returns a dict: ``r``, ``n`` (window volumes, shape 2 S + 1), ``eligible``, ``n_max``, ``peak``
    (the shift, or None), ``peak_window`` (its window index), ``status``, ``shifts``."""
    shape, ndim = F.shape, F.ndim
    S = default_shifts(shape, max_shift)
    min_overlap = 4 ** ndim if min_overlap is None else int(min_overlap)
    vF, vM = validity(F, fixed_mask, valid_above[0]), validity(M, moving_mask, valid_above[1])
    window = [2 * s + 1 for s in S]
    n, num, den = (a.reshape(window) for a in brute_force_at(F, M, itertools.product(*[range(-k, k + 1) for k in S]), fixed_mask, moving_mask, valid_above))
    tol = 1e3 * FLT_EPS * den.max()
    den_ok = den > tol
    r = np.clip(np.where(den_ok, num / np.where(den_ok, den, 1.0), 0.0), -1.0, 1.0)
    eligible, n_max, peak_w, status = select(F, M, vF, vM, r, n, den_ok, overlap_ratio, min_overlap)
    return {"r": r, "n": n, "eligible": eligible, "n_max": n_max, "peak_window": peak_w, "status": status, "shifts": S,
            "peak": None if peak_w is None else [int(p) - s for p, s in zip(peak_w, S)]}


def fft_float64(F, M, fixed_mask=None, moving_mask=None, valid_above=(None, None), overlap_ratio=0.3, min_overlap=None, max_shift=None):
    """The definition through transforms, in float64, for windows the brute force cannot afford: each crop centred and scaled over its
    valid voxels (``(v - mean) / range``; r does not depend on either), the six correlations by ``numpy.fft`` on the padded shape,
    then the window arithmetic of the device chain (``rint(N)``, ``max(N, 1)``, the clamps at 0, the ``1e3 FLT_EPS`` rule, the clip)
    and ``select``.  The result dict of ``brute_force`` plus ``den`` (of the scaled crops) and ``tol`` (the bound it is held against)."""
    shape, ndim = F.shape, F.ndim
    S = default_shifts(shape, max_shift)
    P = padded_shape(shape, S)
    min_overlap = 4 ** ndim if min_overlap is None else int(min_overlap)
    vF, vM = validity(F, fixed_mask, valid_above[0]), validity(M, moving_mask, valid_above[1])

    def centred(im, v):
        out = np.zeros(shape)
        if v.any():
            vals = im[v].astype(np.float64)
            rng = vals.max() - vals.min()
            out[v] = (vals - vals.mean()) / (rng if rng > 0 else 1.0)
        return out

    f, g = centred(F, vF), centred(M, vM)
    axes = tuple(range(ndim))
    spec = {k: np.fft.rfftn(a, s=P, axes=axes) for k, a in (("f", f), ("g", g), ("vF", vF.astype(np.float64)), ("vM", vM.astype(np.float64)), ("f2", f * f), ("g2", g * g))}
    idx = np.ix_(*[np.arange(-s, s + 1) % p for s, p in zip(S, P)])
    corr = lambda a, b: np.fft.irfftn(np.conj(spec[a]) * spec[b], s=P, axes=axes)[idx]      # sum_x a(x) b(x + s) on the window
    N, cFM, cF, cM, cF2, cM2 = corr("vF", "vM"), corr("f", "g"), corr("f", "vM"), corr("vF", "g"), corr("f2", "vM"), corr("vF", "g2")
    nr = np.rint(N)
    nc = np.maximum(nr, 1.0)
    den = np.sqrt(np.maximum(cF2 - cF * cF / nc, 0.0) * np.maximum(cM2 - cM * cM / nc, 0.0))
    num = cFM - cF * cM / nc
    tol = 1e3 * FLT_EPS * den.max()
    den_ok = den > tol
    r = np.clip(np.where(den_ok, num / np.where(den_ok, den, 1.0), 0.0), -1.0, 1.0)
    n = nr.astype(np.int64)
    eligible, n_max, peak_w, status = select(F, M, vF, vM, r, n, den_ok, overlap_ratio, min_overlap)
    return {"r": r, "n": n, "eligible": eligible, "n_max": n_max, "peak_window": peak_w, "status": status, "shifts": S, "padded_shape": P,
            "den": den, "tol": tol, "peak": None if peak_w is None else [int(p) - s for p, s in zip(peak_w, S)]}


def float32_chain(F, M, fixed_mask=None, moving_mask=None, valid_above=(None, None), overlap_ratio=0.3, min_overlap=None, max_shift=None,
                  centre=True):
    """The device chain restated in float32 / complex64 numpy (numpy >= 2 transforms complex64 in single precision): the same
    centring, the same packed transforms and two-for-one separation, the same window arithmetic.  Same result dict, plus ``n_raw``:
    N of the window before ``rint``.  ``centre=False`` leaves the mean in (what the chain would be without its statistics pass: the
    tests show on data with an offset that the centring is needed)."""
    f32, c64 = np.float32, np.complex64
    shape, ndim = F.shape, F.ndim
    S = default_shifts(shape, max_shift)
    P = padded_shape(shape, S)
    min_overlap = 4 ** ndim if min_overlap is None else int(min_overlap)
    vF, vM = validity(F, fixed_mask, valid_above[0]), validity(M, moving_mask, valid_above[1])

    def centred(im, v):
        out = np.zeros(shape, f32)
        if v.any():
            vals = im[v].astype(f32)
            mu = f32(vals.astype(np.float64).sum() / v.sum()) if centre else f32(0)
            rng = f32(vals.max() - vals.min())
            out[v] = (vals - mu) / (rng if rng > 0 else f32(1))
        return out

    f, g = centred(F, vF), centred(M, vM)

    def packed(a, b):
        z = np.zeros(P, c64)
        z[tuple(slice(0, m) for m in shape)] = a.astype(f32) + 1j * b.astype(f32)
        z = np.fft.fftn(z)
        assert z.dtype == c64
        m = np.roll(z[tuple(slice(None, None, -1) for _ in P)], 1, axis=tuple(range(ndim)))      # Z(-k)
        return (f32(0.5) * (z + np.conj(m))).astype(c64), (c64(-0.5j) * (z - np.conj(m))).astype(c64)

    sf, sg = packed(f, g)
    svF, svM = packed(vF, vM)
    sf2, sg2 = packed(f * f, g * g)
    scale = f32(1.0 / np.prod(P))

    def pair(a0, b0, a1, b1):
        x = np.fft.ifftn(((np.conj(a0) * b0 + 1j * (np.conj(a1) * b1)) * scale).astype(c64), norm="forward")
        assert x.dtype == c64
        return x.real.astype(f32), x.imag.astype(f32)

    N, cFM = pair(svF, svM, sf, sg)
    cF, cM = pair(sf, svM, svF, sg)
    cF2, cM2 = pair(sf2, svM, svF, sg2)
    idx = np.ix_(*[np.arange(-s, s + 1) % p for s, p in zip(S, P)])
    N, cFM, cF, cM, cF2, cM2 = (a[idx] for a in (N, cFM, cF, cM, cF2, cM2))
    nr = np.rint(N)
    nc = np.maximum(nr, f32(1))
    dF = np.maximum(cF2 - cF * cF / nc, f32(0))
    dM = np.maximum(cM2 - cM * cM / nc, f32(0))
    den = np.sqrt(dF * dM)
    num = cFM - cF * cM / nc
    assert den.dtype == f32 and num.dtype == f32
    tol = f32(1e3) * f32(FLT_EPS) * den.max()
    den_ok = den > tol
    r = np.clip(np.where(den_ok, num / np.where(den_ok, den, f32(1)), f32(0)), f32(-1), f32(1)).astype(f32)
    n = nr.astype(np.int64)
    eligible, n_max, peak_w, status = select(F, M, vF, vM, r, n, den_ok, overlap_ratio, min_overlap)
    return {"r": r, "n": n, "eligible": eligible, "n_max": n_max, "peak_window": peak_w, "status": status, "shifts": S, "padded_shape": P,
            "n_raw": N, "peak": None if peak_w is None else [int(p) - s for p, s in zip(peak_w, S)]}


def subpixel(r, eligible, peak_w):
    """Per axis the parabola vertex through r at the peak and its two axis neighbours (float64), clamped to +-0.5; 0 where a
    neighbour is outside the window or not eligible, or the curvature is not negative.  Also returns the curvatures (NaN where
    there is no triple)."""
    delta, curv = [], []
    for d in range(r.ndim):
        lo, hi = list(peak_w), list(peak_w)
        lo[d] -= 1
        hi[d] += 1
        if lo[d] < 0 or hi[d] >= r.shape[d] or not (eligible[tuple(lo)] and eligible[tuple(hi)]):
            delta.append(0.0)
            curv.append(np.nan)
            continue
        l, c, h = float(r[tuple(lo)]), float(r[tuple(peak_w)]), float(r[tuple(hi)])
        k = l - 2.0 * c + h
        curv.append(k)
        delta.append(float(np.clip(0.5 * (l - h) / k, -0.5, 0.5)) if k < 0 else 0.0)
    return delta, curv


def unmasked_peak(F, M, vF, vM, max_shift=None, **kwargs):
    """What the same correlation finds without masks on the zero-filled crops (every voxel valid): the case the masks are for."""
    return brute_force(np.where(vF, F, 0).astype(np.float32), np.where(vM, M, 0).astype(np.float32), max_shift=max_shift, **kwargs)["peak"]
