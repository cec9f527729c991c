"""Measurements of the non-rigid refinement kernels on one GPU:

  1. mvs_block_match on one face overlap of the north-star geometry: two resident 512^3 uint16 tiles, an overlap grid of
     512 x 512 x 56, the default block (12) and radius (3) of fit_fields -- 9245 blocks of 343 shifts, in the wrapper's batches;
  2. mvs_field_warp of one resident 512^3 uint16 tile with 4 x 4 x 4 cells, next to mvs_intensity_apply (apply_maps) on the same
     tile in the same process: the yardstick of a kernel that reads and writes a tile once.

    python tools/nonrigid_probe.py --out profiles/nonrigid_probe.txt [--tile 512] [--overlap 56]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _intensity_ops, _lib, _nonrigid_ops, nonrigid  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402


def median_ms(fn, warmup=2, repeats=5):
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
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=56)
    args = ap.parse_args()
    _lib.init(0)
    n, ov = args.tile, args.overlap
    rng = np.random.default_rng(0)
    scene = rng.integers(0, 60000, size=(n, n, 2 * n - ov), dtype=np.uint16)
    fixed = DeviceArray.from_host(np.ascontiguousarray(scene[..., :n]))
    moving = DeviceArray.from_host(np.ascontiguousarray(scene[..., n - ov:]))
    lines = []

    grid = (n, n, ov)
    fixed_affine, moving_affine = (np.eye(3), np.array([0.0, 0.0, float(n - ov)])), (np.eye(3), np.zeros(3))
    block, radius = (12, 12, 12), (3, 3, 3)
    blocks = nonrigid.plan_blocks(grid, block, fixed_affine, moving_affine, (n, n, n), (n, n, n), (4, 4, 4), (4, 4, 4))
    spent = []

    def match():
        # the kernel time of every batch of the call: the wrapper's loop, one batch at a time
        total, limit = 0.0, _lib.MVS_BLOCKMATCH_MAX_RESULT_BYTES // (_nonrigid_ops.n_shifts(radius) * 48)
        for b0 in range(0, len(blocks), limit):
            out = _nonrigid_ops.block_match(fixed, moving, fixed_affine, moving_affine, blocks[b0:b0 + limit], radius)
            total += _lib.last_kernel_ms(0)
        spent.append(total)
        return out

    med, lo, hi, _ = median_ms(match)
    shifts = _nonrigid_ops.n_shifts(radius)
    pairs = float(np.prod(grid)) * shifts
    kernel = statistics.median(spent[-5:])
    lines.append(f"mvs_block_match, grid {grid}, block {block}, radius {radius}: {len(blocks)} blocks x {shifts} shifts; wall median {med:.1f} ms "
                 f"(min {lo:.1f}, max {hi:.1f}) of 5 after 2 warm-up calls, kernels {kernel:.1f} ms -> {pairs / kernel / 1e6:.1f} G sample pairs / s; "
                 f"the rest is the download of {len(blocks) * shifts * 48 / 1e6:.0f} MB of moments into pageable memory and the wrapper")

    out = DeviceArray.empty((n, n, n), np.uint16)
    field = rng.uniform(-1.5, 1.5, (4, 4, 4, 3)).astype(np.float32)
    coeff = np.stack([rng.random((4, 4, 4)) * 0.2 + 0.9, rng.random((4, 4, 4)) * 50], axis=-1).astype(np.float32)
    gb = 2 * fixed.nbytes / 1e9
    results = {}
    for name, fn in {"mvs_intensity_apply (apply_maps), out of place": lambda: _intensity_ops.apply_map(fixed, coeff, out=out),
                     "mvs_field_warp (apply_fields)": lambda: _nonrigid_ops.warp_field(fixed, field, out=out)}.items():
        med, lo, hi, kernel = median_ms(fn, warmup=3, repeats=10)
        results[name] = kernel
        lines.append(f"{name:48s} {n}^3 uint16, 4 x 4 x 4 cells: wall median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of 10 after 3 warm-up calls, "
                     f"kernel {kernel:.3f} ms, {gb:.3f} GB read + written -> {gb / kernel * 1e3:.0f} GB/s")
    a, w = results["mvs_intensity_apply (apply_maps), out of place"], results["mvs_field_warp (apply_fields)"]
    lines.append(f"warp / apply kernel time: {w / a:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
