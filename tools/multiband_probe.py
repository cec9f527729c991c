"""Multi-band fusion on one chunk, by device events: a 256^3 chunk with 2, 4 and 8 float32 views and a 4096^2 chunk with 2, all at
n_levels = 3.  Per configuration one JSON line with three times (median of the timed runs, ms between the events each entry point
records around its kernels, stacks resident on the device, result left there):

  prologue_ms   the shared prologue alone: mvs_resample + mvs_blend_weights of every view (what every stack-based fusion pays)
  multiband_ms  mvs_multiband_fuse: prepare, REDUCE and collapse of every level
  deconv1_ms    mvs_mv_deconv with n_iterations = 1 on the same stacks (default 9-voxel PSF): a yardstick of a comparable pass count

and the bytes model of the chain (csrc/mvs_multiband.hip; DESIGN.md has the terms), its rate and the share of the HBM peak.

    python tools/multiband_probe.py [--reps 5] [--small]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BPS = 8.0e12      # spec
COPY_BPS = 6.29e12         # measured copy ceiling


def level_sizes(shape, levels, origin=0):
    """Samples of a plane per level (the rule of csrc/mvs_multiband_plan.h)."""
    top = max(levels)
    ext = [(origin, n) for n in shape]
    sizes = [int(np.prod([n for _, n in ext]))]
    for l in range(top):
        nxt = []
        for (s, n), lv in zip(ext, levels):
            if lv > l:
                lo, hi = -((-(s - 2)) // 2), (s + n + 1) // 2
                nxt.append((lo, hi - lo + 1))
            else:
                nxt.append((s, n))
        ext = nxt
        sizes.append(int(np.prod([n for _, n in ext])))
    return sizes


def bytes_model(shape, levels, V):
    """HBM bytes the chain has to move, per kernel family (coarse re-reads inside a level are served by L2 and not counted)."""
    s = level_sizes(shape, levels)
    prepare = s[0] * (2 * V * 4 + 4 + V * 4 + 1)                 # read V, B once; write F0, D_v, the winner map
    reduce_ = 0
    for l in range(len(s) - 1):
        reduce_ += (V * 4 + (V * 4 if l else 1)) * s[l] + 2 * V * 4 * s[l + 1]      # read gD_l, gA_l (level 0: the map); write both of l + 1
    collapse = 0
    for l in range(len(s) - 1, 0, -1):
        up = s[l + 1] if l + 1 < len(s) else 0
        collapse += 2 * V * 4 * s[l] + (V + 1) * 4 * up + 4 * s[l]                 # read gD_l, gA_l, gD_{l+1}, r_{l+1}; write r_l
    out = s[0] * (4 + 1 + 4 + 4) + (len(s) > 1) * (2 * 4) * s[1]                     # read F0, map, the winner's D_0, (gD_1 winner, r_1); write the result
    return {"prepare": prepare, "reduce": reduce_, "collapse": collapse, "out": out, "total": prepare + reduce_ + collapse + out}


def _stacks(V, shape, device):
    """Device stacks (V, *shape): views that disagree by a gain and noise, each NaN outside a box of its own; ramp weights."""
    from multiview_stitcher_amd.device import DeviceArray

    rng = np.random.default_rng(0)
    base = rng.random(shape, dtype=np.float32) * np.float32(10) + np.float32(100)
    nx = shape[-1]
    x = np.arange(nx, dtype=np.float32)
    views = np.empty((V,) + tuple(shape), np.float32)
    weights = np.empty((V,) + tuple(shape), np.float32)
    span = int(nx * 0.7)
    for v in range(V):
        lo = int(round((nx - span) * (v / max(1, V - 1))))
        views[v] = base * np.float32(1.0 + 0.03 * v)
        views[v][..., :lo] = np.nan
        views[v][..., lo + span:] = np.nan
        weights[v] = np.clip(np.minimum(x - lo + 1, lo + span - x) / np.float32(64), 0, 1)
    return DeviceArray.from_host(views, device), DeviceArray.from_host(weights, device)


def _median_kernel_ms(fn, reps, device):
    from multiview_stitcher_amd import _lib

    ts = []
    for k in range(reps + 2):
        ms = fn()
        _lib.synchronize(device)
        if ms is None:
            ms = _lib.last_kernel_ms(device)
        if k >= 2:
            ts.append(ms)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="64^3 and 512^2 instead (a check of the script, not a measurement)")
    a = ap.parse_args()
    from multiview_stitcher_amd import _lib, multiband, mv_deconv, transformation, weights
    from multiview_stitcher_amd.device import DeviceArray

    dev = 0
    lib = _lib.init(dev)
    n3, n2 = (64, 512) if a.small else (256, 4096)
    for shape, V in [((n3,) * 3, 2), ((n3,) * 3, 4), ((n3,) * 3, 8), ((n2, n2), 2)]:
        ndim = len(shape)
        levels = [3] * ndim
        views, blend = _stacks(V, shape, dev)
        sdims = ["z", "y", "x"][-ndim:]
        bb = {"origin": {d: 0.0 for d in sdims}, "spacing": {d: 1.0 for d in sdims}, "shape": dict(zip(sdims, shape))}
        tile = DeviceArray.from_host(np.full(shape, 7, np.uint16), dev)

        def prologue():
            total = 0.0
            for _ in range(V):
                transformation.resample_array(tile, np.eye(ndim), np.full(ndim, 0.25), shape, order=1, cval=np.nan, device=dev)
                _lib.synchronize(dev)
                total += _lib.last_kernel_ms(dev)
                wview = _lib.mvs_view_t()
                weights.fill_view_weights(wview, bb, np.eye(ndim + 1), np.zeros(ndim), np.ones(ndim))
                rc = lib.mvs_blend_weights(dev, C.byref(wview), ndim, _lib.i64x3(transformation.shape3(shape)), C.c_void_p(blend_scratch.ptr),
                                           _lib.MVS_MEM_DEVICE)
                _lib.check(rc, dev, "mvs_blend_weights")
                total += _lib.last_kernel_ms(dev)
            return total

        blend_scratch = DeviceArray.empty(shape, np.float32, dev)
        line = {"probe": "multiband", "shape": list(shape), "V": V, "n_levels": 3}
        line["prologue_ms"] = round(_median_kernel_ms(prologue, a.reps, dev), 4)
        del blend_scratch, tile
        run = lambda: multiband._run(views, blend, ndim, [0] * (3 - ndim) + levels, [0, 0, 0], [0] * ndim, np.float32, True, dev) and None
        line["multiband_ms"] = round(_median_kernel_ms(run, a.reps, dev), 4)
        model = bytes_model(shape, levels, V)
        t = line["multiband_ms"] / 1e3
        line["bytes_model"] = model
        line["model_tbps"] = round(model["total"] / t / 1e12, 3)
        line["share_hbm_peak"] = round(model["total"] / t / HBM_PEAK_BPS, 4)
        line["share_copy_ceiling"] = round(model["total"] / t / COPY_BPS, 4)
        kern = mv_deconv._kernels(V, ndim, None, "EFFICIENT_BAYESIAN", None, 0.8, 0.5)

        def deconv():
            # (measured last: the deconvolution masks and normalises `blend` in place, which later runs find done already)
            mv_deconv._run(views, blend, ndim, kern, 1, 0.0, 1e-4, 0, [0] * ndim, np.float32, True, dev, prepare_weights=True)

        line["deconv1_ms"] = round(_median_kernel_ms(deconv, a.reps, dev), 4)
        print(json.dumps(line), flush=True)
        del views, blend


if __name__ == "__main__":
    main()
