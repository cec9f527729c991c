"""Multi-band pyramid fusion on the HIP backend (Burt & Adelson 1983; what enblend and OpenCV's stitcher do).

``multi_band_fusion`` is a ``fusion_func`` of ``fuse()`` / ``fuse_np``: every pyramid band of the views' disagreement is blended over a
zone as wide as its wavelength, so fine structure in an overlap comes from ONE view while illumination is blended widely.  All voxel
work runs on the GPU behind ``mvs_multiband_fuse`` (csrc/mvs_multiband.hip).  There is no CPU fallback.

The definition.  Inputs ``V`` (n_views, [z,] y, x) float32 with NaN = outside the view, ``B`` raw blending weights >= 0 of the same
shape, ``n_levels`` (an int, or a dict giving every spatial dim its own count L_d >= 0; 2D data has a z count of 0) and
``index_origin`` (the global output-grid index of the array's first sample per axis, default 0).

Pointwise: ``m_v = isfinite(V_v)``; ``w_v = m_v ? B_v : 0``; ``cov = sum w > 0``; ``W_v = w_v / sum w`` where ``cov``, else 0;
``I_v = m_v ? V_v : 0``; ``F0 = sum_v W_v I_v``; ``D_v = m_v ? I_v - F0 : 0``; ``A_v = cov && v == argmax_u w_u`` (the lowest index wins
ties; the float32 values themselves are compared).

Pyramid: level l+1 decimates axis d only if ``L_d > l``; ``L = max_d L_d``.  REDUCE along a decimated axis: taps [1,4,6,4,1]/16,
samples kept at GLOBAL even indices, samples outside the array 0; level l+1 holds EVERY coarse sample whose 5-tap window meets level
l's extent [s, s+n): K from ceil((s-2)/2) to floor((s+n+1)/2).  EXPAND along a decimated axis: global even g = 2K:
``(c[K-1] + 6 c[K] + c[K+1]) / 8``; odd g = 2K+1: ``(c[K] + c[K+1]) / 2``; missing coarse samples 0.  Both separable, axis order z, y, x.

Blend and collapse, from l = L down to 0, with gD, gA the reduced D_v, A_v: ``Ahat_{v,l} = gA_{v,l} / sum_u gA_{u,l}`` where the sum
is > 0, else 0; ``lap_{v,l} = gD_{v,l} - EXPAND(gD_{v,l+1})`` (top level: ``gD_{v,L}``);
``r_l = sum_v Ahat_{v,l} lap_{v,l} + EXPAND(r_{l+1})``, summed in view order.  Result: ``cov ? F0 + r_0 : 0``; float32 is left as it
is, integer outputs are rounded half to even and saturated to the dtype's range (band overshoot can leave it).

Consequences: where the views agree, or only one covers, the result is ``F0``; ``n_levels = 0`` is the hard-seam mosaic; the result
at a voxel depends on inputs within ``4 (2^L_d - 1)`` voxels per axis -- ``required_overlap``, the halo ``fuse()`` gives every chunk, with
which chunked and unchunked results of one stack are equal bit for bit (REDUCE is anchored at global indices through ``index_origin``).
Known limit: with fractional tile offsets the blend weights of two chunkings can differ in the last bit, so a tie on the seam midline
may pick the other view in one chunking.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._stack_ops import run_stack_call, stack_dims, stack_inputs

MAX_LEVELS = _lib.MVS_MULTIBAND_MAX_LEVELS
MAX_VIEWS = _lib.MVS_MULTIBAND_MAX_VIEWS
_DIMS = ("z", "y", "x")


def _levels3(n_levels, ndim):
    """``n_levels`` (an int, or a dict with a count per spatial dim) as counts for z, y, x (2D: z = 0)."""
    sdims = _DIMS[3 - ndim:]
    if isinstance(n_levels, dict):
        if sorted(n_levels) != sorted(sdims):
            raise ValueError(f"n_levels must have one entry per spatial dim {list(sdims)}")
        counts = [n_levels[d] for d in sdims]
    else:
        counts = [n_levels] * ndim
    for n in counts:
        if isinstance(n, bool) or int(n) != n or not 0 <= int(n) <= MAX_LEVELS:
            raise ValueError(f"n_levels: every count must be an integer in 0..{MAX_LEVELS}, got {n_levels!r}")
    return [0] * (3 - ndim) + [int(n) for n in counts]


def _origin3(index_origin, ndim):
    """``index_origin`` (None, a sequence per spatial axis, or a dict per spatial dim) as integers for z, y, x."""
    if index_origin is None:
        return [0, 0, 0]
    sdims = _DIMS[3 - ndim:]
    vals = [index_origin[d] for d in sdims] if isinstance(index_origin, dict) else list(np.atleast_1d(index_origin))
    if len(vals) != ndim or any(int(v) != v for v in vals):
        raise ValueError(f"index_origin must be one integer per spatial axis {list(sdims)}")
    return [0] * (3 - ndim) + [int(v) for v in vals]


def _run(views, weights, ndim, levels3, origin3, trim, out_dtype, out_on_device, device, out=None):
    """mvs_multiband_fuse on device float32 stacks (V, *S): the fused chunk, trimmed by ``trim`` (per spatial axis) and cast to
    ``out_dtype``; a DeviceArray or a numpy array.  ``out``: a contiguous DeviceArray of the result shape and dtype to write into
    (with ``out_on_device``)."""
    lib = _lib.init(device)

    def call(shape3, t3, out_dtype_code, out_ptr, out_mem):
        opts = _lib.mvs_multiband_opts_t()
        opts.levels[:] = levels3
        opts.index_origin[:] = origin3
        opts.trim[:] = t3
        opts.out_dtype = out_dtype_code
        opts.flags = 0
        return lib.mvs_multiband_fuse(device, C.c_void_p(views.ptr), C.c_void_p(weights.ptr), views.shape[0], _lib.i64x3(shape3), ndim, C.byref(opts),
                                      C.c_void_p(out_ptr), out_mem)

    return run_stack_call("mvs_multiband_fuse", views, ndim, trim, out_dtype, out_on_device, device, out, call)


def multi_band_fusion(transformed_views, blending_weights, n_levels=3, index_origin=None, device=0):
    """Multi-band fusion of resampled views on the GPU (the module docstring has the definition).

    ``transformed_views`` / ``blending_weights``: (n_views, [z,] y, x), NaN in a view = outside it, raw weights >= 0.  numpy inputs
    return numpy in the views' dtype (integers rounded half to even and saturated); contiguous float32 ``DeviceArray`` inputs return
    a ``DeviceArray`` without a host round trip.  ``n_levels``: an int or a dict per spatial dim, each count in 0..6 (0 = the hard-seam
    mosaic).  ``index_origin``: the global output-grid index of the array's first sample per axis (a sequence or a dict; default 0):
    chunks of one stack that pass their own agree bit for bit where each holds ``required_overlap`` voxels around a result.  At most
    254 views."""
    name = "multi_band_fusion"
    n_views, ndim = stack_dims(name, transformed_views, blending_weights)
    if not 1 <= n_views <= MAX_VIEWS:
        raise ValueError(f"multi_band_fusion takes 1..{MAX_VIEWS} views, got {n_views}")
    levels3, origin3 = _levels3(n_levels, ndim), _origin3(index_origin, ndim)      # (their errors come before any upload)
    views, weights, ndim, out_dtype, on_dev, cast_dtype = stack_inputs(name, transformed_views, blending_weights, device)
    res = _run(views, weights, ndim, levels3, origin3, [0] * ndim, out_dtype, on_dev, device)
    return res if cast_dtype is None else res.astype(cast_dtype, copy=False)


def _required_overlap(func_kwargs):
    """Chunk halo of the multi-band fusion: ``4 (2^n_levels - 1)`` voxels (n_levels defaults to 3), per dim when ``n_levels`` is a
    dict."""
    n_levels = (func_kwargs or {}).get("n_levels", 3)
    if isinstance(n_levels, dict):
        return {d: 4 * (2 ** int(n) - 1) for d, n in n_levels.items()}
    return 4 * (2 ** int(n_levels) - 1)


multi_band_fusion.required_overlap = _required_overlap
