"""Wall and kernel time of registration.masked_correlation_registration on one GPU, next to phase_correlation_registration on the
same crops (masked correlation): a 3D crop of the pair loop's size (51 x 256 x 256, NaN wedges in both crops, resident
on the device) with a bounded max_shift.  The chain is three forward and three inverse transforms of the padded volume plus five
elementwise passes; the ratio to the phase correlation is what this records.

    python tools/masked_corr_probe.py --out profiles/masked_corr_probe.txt [--shape 51 256 256] [--max-shift 12]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _lib, _masked_corr_ops, registration  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402


def median_ms(fn, warmup=2, repeats=7):
    for _ in range(warmup):
        fn()
    times, kernel = [], []
    for _ in range(repeats):
        _lib.synchronize(0)
        t0 = time.perf_counter()
        fn()
        _lib.synchronize(0)
        times.append((time.perf_counter() - t0) * 1e3)
        kernel.append(_lib.last_kernel_ms(0))
    return statistics.median(times), min(times), max(times), statistics.median(kernel)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, nargs=3, default=(51, 256, 256))
    ap.add_argument("--max-shift", type=int, default=12)
    args = ap.parse_args()
    _lib.init(0)
    shape, offset = tuple(args.shape), (2, -5, 7)
    rng = np.random.default_rng(0)
    pad = 8
    big = rng.random([s + 2 * pad for s in shape]).astype(np.float32)
    for axis in range(3):                              # a cheap smoothing: structure at a few voxels
        big = (np.roll(big, 1, axis) + big + np.roll(big, -1, axis)) / 3.0
    F = np.ascontiguousarray(big[tuple(slice(pad, pad + s) for s in shape)])
    M = np.ascontiguousarray(big[tuple(slice(pad - k, pad - k + s) for s, k in zip(shape, offset))])
    ii = np.indices(shape).astype(np.float32)
    u, v = ii[2] / shape[2], ii[1] / shape[1]
    F[(u + v) <= 0.35] = np.nan
    M[(u - v) >= 0.6] = np.nan
    dF, dM = DeviceArray.from_host(F), DeviceArray.from_host(M)
    shifts = _masked_corr_ops.per_axis_shift(args.max_shift, shape)
    padded = _masked_corr_ops.padded_shape(shape, shifts)

    found = {}

    def masked():
        found["masked"] = registration.masked_correlation_registration(dF, dM, max_shift=args.max_shift)

    def phase():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            found["phase"] = registration.phase_correlation_registration(dF, dM)

    lines = [f"crops {shape} float32 on the device, NaN wedges, planted shift {offset}; max_shift {args.max_shift} -> padded {padded} = "
             f"{int(np.prod(padded))} voxels ({int(np.prod(padded)) / np.prod(shape):.2f} x the crop), three complex64 volumes = "
             f"{3 * 8 * int(np.prod(padded)) / 1e6:.0f} MB"]
    results = {}
    for name, fn in (("masked_correlation_registration", masked), ("phase_correlation_registration", phase)):
        med, lo, hi, kernel = median_ms(fn)
        results[name] = (med, kernel)
        res = found["masked" if fn is masked else "phase"]
        t = res["affine_matrix"][:-1, -1] if isinstance(res, dict) else res
        lines.append(f"{name:34s} wall median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of 7 after 2 warm-up calls; last timed kernel span {kernel:.3f} ms; "
                     f"shift {np.round(np.asarray(t, dtype=np.float64), 3).tolist()}, quality {res['quality'] if isinstance(res, dict) else None}")
    m, p = results["masked_correlation_registration"], results["phase_correlation_registration"]
    lines.append(f"masked / phase wall time: {m[0] / p[0]:.2f}   (the masked chain's kernel span covers the whole call; the phase correlation's last "
                 f"timed span covers only its last library call)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
