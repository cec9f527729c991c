"""The numpy / scipy restatement of ``fusion.fuse_np(..., view_weights=)`` (mvs_fuse_chunk_weighted), built from the pieces of
``oracle.fuse_oracle``: ``transform_array`` for the views, ``get_blending_weights`` and ``normalize_weights`` for the blend.

Per view the weight tile ``W`` (uint8, values above 252 counted as 252) is resampled onto the chunk as
``scipy.ndimage.affine_transform(W.astype(float32) / 252, order=1, mode="nearest")`` under the view's own affine, with the tile's
own origin and spacing; a view is set to NaN where that is 0, and the weighted average weighs it with blend weight x tile weight.
Max and simple average run over what is left."""
import warnings

import numpy as np
from scipy.ndimage import affine_transform

from oracle import fuse_oracle as fo

FULL_WEIGHT = 252.0


def resample_weight(tile, param, out_bb):
    """``m`` of one view on the chunk: float32; ``tile`` = {"data", "origin", "spacing"} or None (1 everywhere)."""
    out_shape = tuple(int(s) for s in out_bb["shape"])
    if tile is None:
        return np.ones(out_shape, dtype=np.float32)
    matrix, offset = fo.transform_params(np.linalg.inv(param), tile["origin"], tile["spacing"], out_bb)
    data = np.minimum(np.asarray(tile["data"]).astype(np.float32), np.float32(FULL_WEIGHT)) / np.float32(FULL_WEIGHT)
    return affine_transform(data, matrix=matrix, offset=offset, output_shape=out_shape, order=1, mode="nearest").astype(np.float32)


def fuse_np(views, params, output_properties, weight_tiles, fusion="weighted_average", trim_overlap_in_pixels=0, interpolation_order=1,
            full_view_bbs=None, blending_widths=None):
    """``(fused, fused float32, debug)``: ``fo.fuse_np(..., return_debug=True)`` with a weight tile per view.  ``debug`` also
    carries ``m``, the resampled tile weights (V, *chunk), untrimmed."""
    ndim = views[0]["data"].ndim
    input_dtype = views[0]["data"].dtype
    if full_view_bbs is None:
        full_view_bbs = [fo.bb(v["origin"], v["spacing"], v["data"].shape) for v in views]
    ims = np.stack([fo.transform_array(v["data"].astype(np.float32), np.linalg.inv(p), v["origin"], b["spacing"], output_properties,
                                       order=interpolation_order, cval=np.nan) for v, p, b in zip(views, params, full_view_bbs)])
    m = np.stack([resample_weight(t, p, output_properties) for t, p in zip(weight_tiles, params)])
    ims = np.where(m == 0, np.float32(np.nan), ims)
    raw = None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)
        if fusion == "weighted_average":
            blend = np.stack([fo.get_blending_weights(output_properties, b, p, blending_widths=blending_widths) for b, p in zip(full_view_bbs, params)])
            raw = (blend * m * ~np.isnan(ims)).astype(np.float32)
            fused = fo.weighted_average_fusion(ims, fo.normalize_weights(raw))
        else:
            fused = fo.FUSION_FUNCS[fusion](ims)
    trim = np.broadcast_to(np.asarray(trim_overlap_in_pixels, dtype=np.int64), (ndim,))
    if np.any(trim > 0):
        fused = fused[tuple(slice(t, -t) if t > 0 else slice(None) for t in trim)]
    fused_f = np.nan_to_num(fused)
    return fused_f.astype(input_dtype), fused_f, {"raw_weights": raw, "views": ims, "trim": trim, "m": m}
