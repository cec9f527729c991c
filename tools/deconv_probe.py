"""Multi-view deconvolution on one default chunk: 256^3 output + 4-voxel halo = 264^3, 10 iterations, V = 2 and 4, for the
default 9^3 PSF (direct call) and the PSF fuse() estimates at spacing 1 (11 x 3 x 3), on the separable and the general
convolution path.  Prints one JSON line: ms per chunk (median of the timed runs, device work only: views and weights
resident, result left on the device), FLOP and HBM bytes from the shapes, share of FP32 peak / copy ceiling, and the
restatement's CPU time (tests/deconv_oracle.py) on a sub-box extrapolated to the chunk.  ``--fuse``: also the wall time
of fuse() of a 2 x 2 x 2 grid of 512^3 uint16 tiles (no bar).

    python tools/deconv_probe.py [--reps 5] [--fuse] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 157.3e12      # FP32 vector peak (FMA = 2 FLOP)
COPY_BPS = 6.29e12         # measured copy ceiling


def _views(V, n, device):
    from multiview_stitcher_amd.device import DeviceArray

    rng = np.random.default_rng(0)
    v = (rng.random((V, n, n, n), dtype=np.float32) * 100 + 10).astype(np.float32)
    v[0, :, :, : n // 4] = np.nan
    w = rng.random((V, n, n, n), dtype=np.float32) + np.float32(0.05)
    w = w * ~np.isnan(v)
    w = (w / w.sum(0)).astype(np.float32)
    return DeviceArray.from_host(v, device), DeviceArray.from_host(w, device)


def _time(fn, reps, device):
    from multiview_stitcher_amd import _lib

    fn()
    _lib.synchronize(device)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        _lib.synchronize(device)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=264)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--fuse", action="store_true")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    from multiview_stitcher_amd import _lib, mv_deconv

    dev = 0
    _lib.init(dev)
    n, it = a.n, a.iterations
    S = n ** 3
    line = {"probe": "deconv", "chunk": [n] * 3, "iterations": it, "runs": []}
    psfs = {"default_9": None, "fuse_estimated_spacing1": {"z": 1.0, "y": 1.0, "x": 1.0}}
    for V in (2, 4):
        views, weights = _views(V, n, dev)
        for pname, spacing in psfs.items():
            kern = mv_deconv._kernels(V, 3, None, "EFFICIENT_BAYESIAN", spacing, 0.8, 0.5)
            k = kern[0].shape[1:]
            for path in ("separable", "general"):
                _lib.set_option("deconv_general", 1 if path == "general" else 0, dev)
                run = lambda: mv_deconv._run(views, weights, 3, kern, it, 0.0, 1e-4, 0, [0, 0, 0], np.float32, True, dev)
                ms = _time(run, a.reps, dev)
                convs = 2 * V * it
                if path == "general":
                    flop = 2.0 * convs * S * int(np.prod(k))
                    # each convolution reads its input once from HBM (planes re-read from L2) and the epilogue's operands
                    hbm = convs * S * 4 * 2 + V * it * S * 4 * (3 + 2)
                else:
                    flop = 2.0 * convs * S * int(sum(k))
                    hbm = convs * S * 4 * 6 + V * it * S * 4 * (3 + 2)
                t = ms / 1e3
                rec = {"V": V, "psf": pname, "kernel": list(k), "path": path, "ms": round(ms, 3), "flop": flop,
                       "hbm_bytes_model": hbm, "tflops": round(flop / t / 1e12, 2), "share_fp32_peak": round(flop / t / PEAK_FLOPS, 4),
                       "hbm_tbps_model": round(hbm / t / 1e12, 2), "share_copy_ceiling": round(hbm / t / COPY_BPS, 4)}
                rec["bound"] = "compute" if rec["share_fp32_peak"] > rec["share_copy_ceiling"] else "memory"
                line["runs"].append(rec)
        _lib.set_option("deconv_general", 0, dev)
        del views, weights
    if not a.no_cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from tests import deconv_oracle as do

        m = 48
        rng = np.random.default_rng(1)
        v = (rng.random((2, m, m, m)) * 100 + 10).astype(np.float32)
        w = np.full((2, m, m, m), 0.5, np.float32)
        t0 = time.perf_counter()
        do.deconvolve(v, w, n_iterations=it)
        cpu = time.perf_counter() - t0
        line["cpu_restatement"] = {"box": [m] * 3, "V": 2, "s": round(cpu, 3), "extrapolated_chunk_s": round(cpu * S / m ** 3, 1)}
    if a.fuse:
        from multiview_stitcher_amd import fusion, sample_data

        sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=(512, 512, 512), tiles=(2, 2, 2), overlap=(32, 32, 32),
                                                        max_jitter=0, dtype=np.uint16)
        t0 = time.perf_counter()
        fused = fusion.fuse(sims, transform_key=sample_data.METADATA_TRANSFORM_KEY, fusion_func=fusion.multi_view_deconvolution,
                            output_chunksize=256)
        shape = list(np.asarray(fused.data).shape)
        line["fuse_2x2x2_512_u16"] = {"s": round(time.perf_counter() - t0, 2), "shape": shape}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
