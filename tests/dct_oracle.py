"""numpy / scipy restatement of weights.content_based_dct (DCT Shannon-entropy fusion weights, Royer et al. 2016) and of
its required_overlap, plus the seeded cases of tests/golden/dct_weights_ref.npz.

The reference's defaults: dct_size=32, exponent=1.0, otf_support_fraction=0.5, output_chunksize=None.
"""
import numpy as np
from scipy.fftpack import dctn
from scipy.ndimage import affine_transform


def clamped_sizes(shape, dct_size=32, output_chunksize=None):
    ndim = len(shape)
    sdims = ["z", "y", "x"][-ndim:]
    sizes = [dct_size[d] for d in sdims] if isinstance(dct_size, dict) else [dct_size] * ndim
    if output_chunksize is not None:
        return tuple(int(min(ds, output_chunksize[d], s)) for ds, d, s in zip(sizes, sdims, shape))
    return tuple(int(min(ds, s)) for ds, s in zip(sizes, shape))


def quality_maps(views, dct_size=32, exponent=1.0, otf_support_fraction=0.5, output_chunksize=None):
    """Raw per-block qualities (n_views, *blocks) before the shift by their minimum over the views."""
    views = np.asarray(views, dtype=np.float32)
    shape = views.shape[1:]
    ds = clamped_sizes(shape, dct_size, output_chunksize)
    nb = tuple(max(1, int(np.ceil(s / d))) for s, d in zip(shape, ds))
    q = np.zeros((len(views),) + nb, np.float32)
    r_o = None if otf_support_fraction is None else otf_support_fraction * min(ds)
    for iv, view in enumerate(views):
        for bi in np.ndindex(nb):
            blk = view[tuple(slice(i * d, min((i + 1) * d, s)) for i, d, s in zip(bi, ds, shape))]
            nan = np.isnan(blk)
            if np.sum(~nan) < 0.2 * blk.size:
                continue
            if nan.any():
                fill = float(np.nanmin(blk))
                blk = np.where(nan, np.float32(fill if fill > 0.0001 else 0.0), blk)
            d = dctn(blk, norm="ortho")
            if r_o is not None:
                l2 = float(np.sqrt(np.sum(d.astype(np.float64) ** 2)))
                if l2 == 0.0:
                    continue
                mask = np.sum(np.indices(d.shape), axis=0) < r_o
                p = np.abs(d[mask]) / np.float32(l2)
                p = p[p > 0]
                h = -float(np.sum(p.astype(np.float64) * np.log2(p).astype(np.float64)))
                v = np.float32((2.0 / r_o**2) * h)
                q[iv][bi] = np.float32(v ** np.float32(exponent)) * np.sign(v)
            else:
                a = np.abs(d)
                dsl1 = np.float32(np.mean(a.astype(np.float64)))
                if dsl1 == 0.0:
                    continue
                p = a / dsl1
                p = p[p > 0]
                h = -float(np.sum(p.astype(np.float64) * np.log2(p).astype(np.float64)))
                with np.errstate(invalid="ignore"):
                    q[iv][bi] = np.power(np.float64(dsl1) * h, float(exponent))      # negative base, fractional exponent: NaN
    return q


def normalize_weights(w):
    wsum = np.nansum(w, axis=0)
    wsum[wsum == 0] = 1
    return w / wsum


def shifted(q):
    """Q - nanmin(Q, axis=0) (the input of the first normalize_weights)."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return q - np.nanmin(q, axis=0)


def content_based_dct(transformed_views, dct_size=32, exponent=1.0, otf_support_fraction=0.5, output_chunksize=None):
    """The weights (n_views, *spatial) float32, as the reference computes them on the host."""
    views = np.asarray(transformed_views, dtype=np.float32)
    shape = views.shape[1:]
    ds = clamped_sizes(shape, dct_size, output_chunksize)
    qn = normalize_weights(shifted(quality_maps(views, dct_size, exponent, otf_support_fraction, output_chunksize)))
    m = np.diag([1.0 / d for d in ds])
    off = [-(d - 1) / (2.0 * d) for d in ds]
    w = np.stack([affine_transform(qv, m, offset=off, output_shape=shape, order=1, mode="nearest") for qv in qn])
    return normalize_weights(w).astype(np.float32)


def required_overlap(kwargs):
    """@requires_overlap(lambda kw: _clamp_overlap(kw["dct_size"], kw["output_chunksize"])) with the defaults merged."""
    kw = {"dct_size": 32, "exponent": 1.0, "otf_support_fraction": 0.5, "output_chunksize": None, **(kwargs or {})}
    ocs = kw["output_chunksize"]
    sdims = sorted(ocs.keys())[::-1]
    ov = kw["dct_size"] if isinstance(kw["dct_size"], dict) else {d: int(kw["dct_size"]) for d in sdims}
    return {d: min(ov[d], ocs[d]) for d in sdims}


def cases():
    """name -> (views (V, *S) float32, kwargs).  Views differ in content so that blocks do not tie in quality."""
    out = {}
    rng = np.random.default_rng(15)

    def pair(shape, sharp=0.7, blur=2.5):
        base = rng.random(shape)
        from scipy.ndimage import gaussian_filter

        a = (gaussian_filter(base, sharp) * 1000 + 100).astype(np.float32)
        b = (gaussian_filter(base, blur) * 1000 + 100).astype(np.float32)
        return np.stack([a, b])

    out["2d_default"] = (pair((70, 90)), {})
    out["2d_dict_edges"] = (pair((45, 53)), {"dct_size": {"y": 16, "x": 12}})
    out["2d_big_dct"] = (pair((20, 24)), {"dct_size": 64})
    out["3d_default"] = (pair((40, 36, 44)), {})
    out["3d_dict"] = (pair((20, 30, 33)), {"dct_size": {"z": 8, "y": 16, "x": 12}, "otf_support_fraction": 0.25})
    out["3d_z1"] = (pair((1, 40, 40)), {"dct_size": 16})
    out["3d_z3"] = (pair((3, 40, 40)), {"dct_size": 16, "otf_support_fraction": 1.0})
    out["otf_exp2"] = (pair((48, 48)), {"dct_size": 16, "exponent": 2.0})
    out["otf_exp05"] = (pair((48, 48)), {"dct_size": 16, "exponent": 0.5})
    out["l1_exp1"] = (pair((48, 40)), {"dct_size": 16, "otf_support_fraction": None})
    out["l1_exp2_3d"] = (pair((16, 24, 24)), {"dct_size": 8, "otf_support_fraction": None, "exponent": 2.0})
    out["chunk_clamp"] = (pair((30, 60, 60)), {"dct_size": 32, "output_chunksize": {"z": 10, "y": 20, "x": 24}})
    # coverage: view 1 covers only the left part (NaN elsewhere: blocks below 20 % are skipped, others NaN-filled with the
    # block minimum, which is > 1e-4); view 2 holds values <= 0 next to its NaN (filled with 0); an all-zero block
    v = pair((64, 64))
    v[0][:, 37:] = np.nan
    v[1] = v[1] - 700.0
    v[1][50:, :20] = np.nan
    v[0][:16, :16] = 0.0
    v[1][:16, :16] = 0.0
    out["nan_fill"] = (v, {"dct_size": 16})
    out["single_view"] = (pair((40, 40))[:1], {"dct_size": 16})
    three = np.concatenate([pair((36, 40)), pair((36, 40))[:1] * 0.5 + 30.0])
    out["three_views"] = (three, {"dct_size": 12})
    return out


def overlap_cases():
    return [
        ({}, {"z": 64, "y": 128, "x": 128}),
        ({"dct_size": 16}, {"y": 100, "x": 8}),
        ({"dct_size": {"z": 4, "y": 48, "x": 64}}, {"z": 16, "y": 32, "x": 128}),
    ]


content_based_dct.required_overlap = required_overlap      # (as the reference's decorator attaches it)
