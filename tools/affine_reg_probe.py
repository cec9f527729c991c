"""Gauss-Newton intensity registration on one 200 x 400 x 400 crop pair with resident inputs.
Prints one JSON line: wall ms (median) of one mvs_affine_normal_eq call (launch + partial sum + wait, as the optimiser pays
it) at full resolution and at bin 2, its bytes per voxel (two float32 reads: 8 B) against the float4-copy ceiling DESIGN.md
quotes, and wall ms, iteration count and corner error of one full affine_registration (rigid, defaults) on a pair whose
moving crop is rotated by 1 deg and shifted.  Warm-up and timed repetitions each run under a time limit: a call that does
not return ends the probe.

    python tools/affine_reg_probe.py [--reps 20] [--limit 120]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_CEILING = 6.29e12      # B/s, measured float4 copy
SHAPE = (200, 400, 400)


class _Limit:
    """SIGALRM after ``seconds``: the default action ends the process."""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def _median_wall_ms(fn, reps, limit):
    with _Limit(limit):
        fn()
    ts = []
    with _Limit(limit):
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=120, help="seconds for the warm-up and for the timed repetitions of each step")
    a = ap.parse_args()
    from scipy import ndimage

    from multiview_stitcher_amd import _affine_reg, _lib, _reg_ops, registration
    from multiview_stitcher_amd.device import DeviceArray

    dev = 0
    _lib.init(dev)
    rng = np.random.default_rng(0)
    pad = 8
    G = ndimage.gaussian_filter(rng.random(tuple(n + 2 * pad for n in SHAPE), dtype=np.float32), 2.0)
    G = (G - G.min()) / (G.max() - G.min())
    F = np.ascontiguousarray(G[tuple(slice(pad, pad + n) for n in SHAPE)])
    a1 = np.deg2rad(1.0)
    A0 = np.array([[1, 0, 0], [0, np.cos(a1), -np.sin(a1)], [0, np.sin(a1), np.cos(a1)]])
    t0 = np.array([0.7, -1.1, 0.9])
    c = (np.array(SHAPE) - 1) / 2.0
    R = np.linalg.inv(A0)
    M = ndimage.affine_transform(G, R, offset=pad + c - R @ t0 - R @ c, output_shape=SHAPE, order=1, mode="nearest").astype(np.float32)
    Fd, Md = DeviceArray.from_host(F, dev), DeviceArray.from_host(M, dev)
    res = {"shape": list(SHAPE)}
    n = float(np.prod(SHAPE))
    ms = _median_wall_ms(lambda: _reg_ops.affine_normal_equations(Fd, Md, A0, t0, 1.0, 0.0, dev), a.reps, a.limit)
    res["normal_eq_ms"] = ms
    res["bytes_per_voxel"] = 8
    res["normal_eq_tb_s"] = 8 * n / (ms * 1e-3) / 1e12
    res["frac_of_copy_ceiling"] = 8 * n / (ms * 1e-3) / COPY_CEILING
    F2, M2 = _reg_ops.bin_mean(Fd, [2, 2, 2], dev), _reg_ops.bin_mean(Md, [2, 2, 2], dev)
    res["normal_eq_bin2_ms"] = _median_wall_ms(lambda: _reg_ops.affine_normal_equations(F2, M2, A0, t0 / 2, 1.0, 0.0, dev), a.reps, a.limit)
    out = {}

    def full():
        out["r"] = registration.affine_registration(Fd, Md, transform_type="rigid", device=dev, return_debug=True)

    res["registration_ms"] = _median_wall_ms(full, max(1, a.reps // 4), a.limit)
    hist = out["r"]["debug"]["history"]
    res["iterations"] = [sum(1 for h in hist if h["level"] == lv) for lv in sorted({h["level"] for h in hist})]
    A, t = _affine_reg.matrix_to_pose(out["r"]["affine_matrix"], SHAPE)
    res["corner_error_px"] = _affine_reg.corner_displacement(A, t, A0, t0, SHAPE)
    res["quality"] = out["r"]["quality"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
