"""numpy restatement of the multi-band fusion (multiview_stitcher_amd.multiband has the definition): any number of spatial dims, any
float dtype (float64 by default; float32 for the conditioning checks), with ``index_origin``.  Every expression is written once and
applied to whole arrays, samples outside an array enter as zeros."""
import numpy as np


def radius(n_levels):
    return 4 * (2 ** int(n_levels) - 1)


def levels_list(n_levels, ndim):
    """Per-axis level counts from an int, a sequence or a dict per spatial dim (2D: no z)."""
    if isinstance(n_levels, dict):
        return [int(n_levels[d]) for d in ("z", "y", "x")[3 - ndim:]]
    if np.ndim(n_levels) == 0:
        return [int(n_levels)] * ndim
    assert len(n_levels) == ndim
    return [int(n) for n in n_levels]


def axis_geometry(start, n, levels, top):
    """[(start, extent)] of levels 0..top of one axis that is decimated ``levels`` times."""
    out = [(int(start), int(n))]
    for l in range(top):
        s, m = out[-1]
        if levels > l:
            lo, hi = -((-(s - 2)) // 2), (s + m + 1) // 2          # ceil((s - 2) / 2), floor((s + m + 1) / 2)
            out.append((lo, hi - lo + 1))
        else:
            out.append((s, m))
    return out


def _take(a, axis, idx):
    return np.take(a, idx, axis=axis)


def reduce_axis(a, axis, s):
    """REDUCE along ``axis`` of an array whose first sample has global index ``s``: (coarse array, its global start)."""
    n = a.shape[axis]
    (_, _), (lo, m) = axis_geometry(s, n, 1, 1)
    front, back = s - (2 * lo - 2), (2 * (lo + m - 1) + 2) - (s + n - 1)
    pad = [(0, 0)] * a.ndim
    pad[axis] = (front, back)
    p = np.pad(a, pad)
    t = [_take(p, axis, np.arange(m) * 2 + j) for j in range(5)]
    six, four, sixteenth = a.dtype.type(6), a.dtype.type(4), a.dtype.type(0.0625)
    return (six * t[2] + four * (t[1] + t[3]) + (t[0] + t[4])) * sixteenth, lo


def expand_axis(c, axis, s_c, s_f, n_f):
    """EXPAND along ``axis`` of a coarse array (global start ``s_c``) onto the fine samples s_f .. s_f + n_f - 1."""
    g = s_f + np.arange(n_f)
    k = g // 2
    lo, hi = int(k.min()) - 1, int(k.max()) + 1
    front, back = max(0, s_c - lo), max(0, hi - (s_c + c.shape[axis] - 1))
    pad = [(0, 0)] * c.ndim
    pad[axis] = (front, back)
    p = np.pad(c, pad)
    base = s_c - front
    a, b, d = (_take(p, axis, k - base + j) for j in (-1, 0, 1))
    even = (c.dtype.type(6) * b + (a + d)) * c.dtype.type(0.125)
    odd = (b + d) * c.dtype.type(0.5)
    shape = [1] * c.ndim
    shape[axis] = n_f
    return np.where((g % 2 == 0).reshape(shape), even, odd)


def reduce_level(a, starts, dec):
    """One REDUCE step of a stack (V, *S): the spatial axes with ``dec`` set, in axis order.  Returns (array, new starts)."""
    starts = list(starts)
    for d, on in enumerate(dec):
        if on:
            a, starts[d] = reduce_axis(a, d + 1, starts[d])
    return a, starts


def expand_level(c, c_starts, f_starts, f_shape, dec, lead=1):
    """One EXPAND step onto a level with starts ``f_starts`` and spatial shape ``f_shape`` (``lead`` leading non-spatial axes)."""
    for d, on in enumerate(dec):
        if on:
            c = expand_axis(c, d + lead, c_starts[d], f_starts[d], f_shape[d])
    return c


def pointwise(V, B, dtype=np.float64):
    """(F0, D, winner, cov): the pointwise part; ``winner`` is the lowest index of the largest masked weight."""
    V, B = np.asarray(V, dtype=dtype), np.asarray(B, dtype=dtype)
    m = np.isfinite(V)
    w = np.where(m, B, dtype(0))
    sw = np.zeros(V.shape[1:], dtype)
    for v in range(len(V)):
        sw = sw + w[v]
    cov = sw > 0
    safe = np.where(cov, sw, dtype(1))
    I = np.where(m, V, dtype(0))
    F0 = np.zeros(V.shape[1:], dtype)
    for v in range(len(V)):
        F0 = F0 + np.where(cov & m[v], (w[v] / safe) * I[v], dtype(0))
    D = np.where(m, I - F0, dtype(0))
    return F0, D, np.argmax(w, axis=0), cov


def multi_band(V, B, n_levels=3, index_origin=None, dtype=np.float64):
    """The float result (``dtype``) of the multi-band fusion of V, B (n_views, *spatial)."""
    dtype = np.dtype(dtype).type
    ndim = np.ndim(V) - 1
    levels = levels_list(n_levels, ndim)
    top = max(levels) if levels else 0
    starts0 = [0] * ndim if index_origin is None else [int(v) for v in index_origin]
    F0, D, winner, cov = pointwise(V, B, dtype)
    A = np.stack([(cov & (winner == v)).astype(dtype) for v in range(len(D))])
    gD, gA, starts = [D], [A], [starts0]
    for l in range(top):
        dec = [levels[d] > l for d in range(ndim)]
        d_next, s_next = reduce_level(gD[-1], starts[-1], dec)
        a_next, _ = reduce_level(gA[-1], starts[-1], dec)
        gD.append(d_next), gA.append(a_next), starts.append(s_next)
    r = None
    for l in range(top, -1, -1):
        dec = [levels[d] > l for d in range(ndim)]
        sum_a = np.zeros(gA[l].shape[1:], dtype)
        for v in range(len(D)):
            sum_a = sum_a + gA[l][v]
        safe = np.where(sum_a > 0, sum_a, dtype(1))
        lap = gD[l] if l == top else gD[l] - expand_level(gD[l + 1], starts[l + 1], starts[l], gD[l].shape[1:], dec)
        acc = np.zeros(gA[l].shape[1:], dtype)
        for v in range(len(D)):
            acc = acc + np.where(sum_a > 0, gA[l][v] / safe, dtype(0)) * lap[v]
        r = acc if l == top else acc + expand_level(r, starts[l + 1], starts[l], gD[l].shape[1:], dec, lead=0)
    return np.where(cov, F0 + r, dtype(0))


def cast(res, out_dtype):
    """The result in ``out_dtype``: floats as they are, integers rounded half to even and saturated."""
    out_dtype = np.dtype(out_dtype)
    if out_dtype.kind == "f":
        return res.astype(out_dtype)
    info = np.iinfo(out_dtype)
    return np.clip(np.rint(res), info.min, info.max).astype(out_dtype)


def chunked(V, B, n_levels, lo, hi, halo, index_origin=None, clip=True, dtype=np.float64, anchored=True):
    """The result on the box [lo, hi) (array indices per axis) computed from a chunk with ``halo`` voxels around it: clipped at the
    array (``clip``) or padded beyond it with NaN views and zero weights.  ``anchored``: the chunk passes its own global start."""
    ndim = np.ndim(V) - 1
    halo = [halo] * ndim if np.ndim(halo) == 0 else list(halo)
    origin = [0] * ndim if index_origin is None else list(index_origin)
    a = [l - h for l, h in zip(lo, halo)]
    b = [u + h for u, h in zip(hi, halo)]
    if clip:
        a = [max(0, v) for v in a]
        b = [min(n, v) for v, n in zip(b, np.shape(V)[1:])]
        Vc, Bc = V[(slice(None),) + tuple(slice(p, q) for p, q in zip(a, b))], B[(slice(None),) + tuple(slice(p, q) for p, q in zip(a, b))]
    else:
        pad = [(0, 0)] + [(max(0, -p), max(0, q - n)) for p, q, n in zip(a, b, np.shape(V)[1:])]
        Vp, Bp = np.pad(np.asarray(V, np.float64), pad, constant_values=np.nan), np.pad(np.asarray(B, np.float64), pad)
        sel = (slice(None),) + tuple(slice(p + f, q + f) for p, q, (f, _) in zip(a, b, pad[1:]))
        Vc, Bc = Vp[sel], Bp[sel]
    start = [o + p for o, p in zip(origin, a)] if anchored else [0] * ndim
    res = multi_band(Vc, Bc, n_levels, start, dtype)
    return res[tuple(slice(l - p, u - p) for l, u, p in zip(lo, hi, a))]
