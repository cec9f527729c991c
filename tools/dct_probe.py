"""DCT-entropy fusion weights on one default chunk: 256^3 output + 32-voxel halo = 320^3, V = 2 resident uint16 tiles.
Prints one JSON line: device ms (median of the timed runs, context events) of the quality pass alone
(mvs_content_dct_weights with the interpolation included, measured on the resampled float32 stack, on the LDS and the
general path), of mvs_fuse_chunk_dct, and of mvs_fuse_chunk with force_generic on the same chunk; the quality pass's
FLOP (3 x ds MACs per voxel and view) and share of FP32 peak; and the restatement's CPU time (tests/dct_oracle.py) on a
(2, 64, 320, 320) sub-box extrapolated to the chunk.

    python tools/dct_probe.py [--reps 5] [--no-cpu]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 157.3e12      # FP32 vector peak (FMA = 2 FLOP)
N, HALO, V, DS = 256, 32, 2, 32


def _median_ms(fn, reps, device):
    from multiview_stitcher_amd import _lib

    fn()
    ts = []
    for _ in range(reps):
        fn()
        _lib.synchronize(device)
        ts.append(_lib.last_kernel_ms(device))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from multiview_stitcher_amd import _lib, fusion, weights
    from multiview_stitcher_amd import spatial_image_utils as si_utils
    from multiview_stitcher_amd.device import DeviceArray

    dev = 0
    lib = _lib.init(dev)
    S = N + 2 * HALO
    rng = np.random.default_rng(0)
    # two overlapping tiles along x, each 320 x 320 x 224, offset by 96 voxels: every chunk voxel is seen by >= 1 view
    tiles = [(rng.random((S, S, 224), dtype=np.float32) * 4000).astype(np.uint16) for _ in range(V)]
    from tests.helpers import squeeze_field

    sims = [squeeze_field(si_utils.get_sim_from_array(t, dims=["z", "y", "x"], translation={"z": 0.0, "y": 0.0, "x": 96.0 * i}))
            for i, t in enumerate(tiles)]
    params = [np.eye(4) for _ in sims]
    sd = ["z", "y", "x"]
    out_bb = {"origin": {d: 0.0 for d in sd}, "spacing": {d: 1.0 for d in sd}, "shape": {d: S for d in sd}}
    fvb = [si_utils.get_stack_properties_from_sim(s) for s in sims]
    out = DeviceArray.empty((N, N, N), np.uint16, dev)
    kw = dict(full_view_bbs=fvb, trim_overlap_in_pixels=HALO, out=out, device=dev)
    res = {"chunk": [S] * 3, "views": V, "dct_size": DS}
    res["fuse_chunk_dct_ms"] = _median_ms(lambda: fusion.fuse_np(sims, params, out_bb, weights_func=fusion.content_based_dct, **kw), a.reps, dev)
    _lib.set_option("force_generic", 1, dev)
    res["fuse_chunk_generic_ms"] = _median_ms(lambda: fusion.fuse_np(sims, params, out_bb, **kw), a.reps, dev)
    _lib.set_option("force_generic", 0, dev)
    res["dct_over_generic"] = res["fuse_chunk_dct_ms"] / res["fuse_chunk_generic_ms"]
    stack = DeviceArray.from_host(rng.random((V, S, S, S), dtype=np.float32) * 4000, dev)
    wout = DeviceArray.empty((V, S, S, S), np.float32, dev)
    opts = weights.dct_opts(3, DS)
    call = lambda: lib.mvs_content_dct_weights(dev, C.c_void_p(stack.ptr), V, _lib.i64x3((S, S, S)), 3, C.byref(opts),  # noqa: E731
                                               C.c_void_p(wout.ptr), None, _lib.MVS_MEM_DEVICE)
    for path in ("lds", "general"):
        _lib.set_option("dct_general", int(path == "general"), dev)
        res[f"weights_{path}_ms"] = _median_ms(call, a.reps, dev)
    _lib.set_option("dct_general", 0, dev)
    flop = 2.0 * 3 * DS * V * S**3
    res["quality_gflop"] = flop / 1e9
    res["weights_lds_peak_frac"] = flop / (res["weights_lds_ms"] * 1e-3) / PEAK_FLOPS
    res["targets"] = {"quality_ms": 1.0, "dct_over_generic": 2.0}
    if not a.no_cpu:
        from tests import dct_oracle as do

        sub = np.asarray(stack.get()[:, :64])
        t = time.perf_counter()
        do.quality_maps(sub, DS)
        res["restatement_cpu_s_chunk"] = (time.perf_counter() - t) * S / 64
    print(json.dumps(res))


if __name__ == "__main__":
    main()
