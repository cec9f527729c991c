"""One iteration of affine_registration(metric="mattes") against one iteration of the squared-residual loop, resident float32 crops.
Per size prints one JSON line: wall ms (median, the launches and the wait as the optimiser pays them) of the joint histogram
(mvs_affine_joint_hist), the gradient reduction (mvs_affine_mi_gradient), the normal equations (mvs_affine_normal_eq: the whole
squared-residual iteration, and the preconditioner of the mattes loop) and their ratio.  The three are timed in alternating rounds
so that a drift of the machine reaches all of them alike.  Warm-up and timed rounds run under a time limit: a call that does not
return ends the probe.

    python tools/affine_mi_probe.py [--sizes 128 256] [--rounds 15] [--bins 32] [--limit 120]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--limit", type=int, default=120, help="seconds for all rounds of one size")
    a = ap.parse_args()
    from scipy import ndimage

    from multiview_stitcher_amd import _affine_reg, _lib, _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    dev = 0
    _lib.init(dev)
    a1 = np.deg2rad(1.0)
    A = np.array([[1, 0, 0], [0, np.cos(a1), -np.sin(a1)], [0, np.sin(a1), np.cos(a1)]])
    t = np.array([0.7, -1.1, 0.9])
    for size in a.sizes:
        shape = (size,) * 3
        rng = np.random.default_rng(0)
        F = ndimage.gaussian_filter(rng.random(shape, dtype=np.float32), 2.0)
        M = np.abs(2.0 * F - 2.0 * np.median(F)).astype(np.float32)          # a relation no gain and offset describes
        Fd, Md = DeviceArray.from_host(F, dev), DeviceArray.from_host(M, dev)
        ranges = _affine_reg.bin_ranges(*_reg_ops.finite_range(Fd, dev)[:2], *_reg_ops.finite_range(Md, dev)[:2], a.bins)
        state = {}

        def hist():
            state["hist"], state["n"] = _reg_ops.affine_joint_hist(Fd, Md, A, t, a.bins, ranges, dev)

        def grad():
            _reg_ops.affine_mi_gradient(Fd, Md, A, t, a.bins, ranges, state["table"], dev)

        def neq():
            _reg_ops.affine_normal_equations(Fd, Md, A, t, 1.0, 0.0, dev)

        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(a.limit)
        hist()
        state["table"] = _affine_reg.mutual_information(state["hist"])[1]
        grad()
        neq()
        times = {"hist": [], "grad": [], "neq": []}
        for _ in range(a.rounds):
            for name, fn in (("neq", neq), ("hist", hist), ("grad", grad)):
                t0 = time.perf_counter()
                fn()
                times[name].append((time.perf_counter() - t0) * 1e3)
        signal.alarm(0)
        med = {k: float(np.median(v)) for k, v in times.items()}
        mi_iter = med["hist"] + med["grad"] + med["neq"]
        print(json.dumps({"shape": list(shape), "bins": a.bins, "joint_hist_ms": med["hist"], "mi_gradient_ms": med["grad"],
                          "normal_eq_ms": med["neq"], "mattes_iteration_ms": mi_iter, "ssd_iteration_ms": med["neq"],
                          "ratio": mi_iter / med["neq"], "n_valid": state["n"],
                          "spread_ms": {k: [float(np.min(v)), float(np.max(v))] for k, v in times.items()}}), flush=True)


if __name__ == "__main__":
    main()
