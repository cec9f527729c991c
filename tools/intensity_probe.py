"""Measurements of the tile intensity harmonisation on one GPU:

  1. mvs_intensity_apply on one resident 512^3 uint16 tile, out of place and in place, next to a device-to-device copy of the same
     bytes timed in the same process (warm-up, repeats, median);
  2. intensity.fit_maps on the north-star geometry (4 x 4 x 4 tiles of 512^3 uint16, 20 % overlap, the 144 face-neighbour pairs),
     wall time split into moments (planning + kernel calls) and solve, for cells = 1 and cells = 4.

    python tools/intensity_probe.py --out profiles/intensity_probe.txt [--tile 512] [--grid 4] [--skip-fit]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _intensity_ops, _lib, intensity  # noqa: E402
from multiview_stitcher_amd import spatial_image_utils as si  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402


def median_ms(fn, warmup=3, repeats=10):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        _lib.synchronize(0)
        t0 = time.perf_counter()
        fn()
        _lib.synchronize(0)
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def apply_leg(n, lines):
    rng = np.random.default_rng(0)
    tile = DeviceArray.from_host(rng.integers(0, 60000, size=(n, n, n), dtype=np.uint16))
    out = DeviceArray.empty((n, n, n), np.uint16)
    out32 = DeviceArray.empty((n, n, n), np.float32)
    coeff = np.stack([rng.random((4, 4, 4)) * 0.2 + 0.9, rng.random((4, 4, 4)) * 50], axis=-1).astype(np.float32)
    gb = 2 * tile.nbytes / 1e9
    legs = {
        "device-to-device copy": lambda: tile.copy_into(out, (0, 0, 0)),
        "apply, out of place": lambda: _intensity_ops.apply_map(tile, coeff, out=out),
        "apply, in place": lambda: _intensity_ops.apply_map(tile, coeff, out=tile),
        "apply, uint16 -> float32": lambda: _intensity_ops.apply_map(tile, coeff, out=out32, out_dtype=np.float32),
    }
    for name, fn in legs.items():
        med, lo, hi = median_ms(fn)
        moved = gb if "float32" not in name else (tile.nbytes + out32.nbytes) / 1e9
        kernel = f", kernel {_lib.last_kernel_ms(0):.3f} ms" if name.startswith("apply") else ""
        lines.append(f"{name:28s} {n}^3 uint16: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of 10 after 3 warm-up calls, "
                     f"{moved:.3f} GB read + written -> {moved / med * 1e3:.0f} GB/s{kernel}")


def fit_leg(n, grid, lines):
    rng = np.random.default_rng(1)
    first = DeviceArray.from_host(rng.integers(0, 60000, size=(n, n, n), dtype=np.uint16))
    step = n - int(round(0.2 * n))
    sims, index = [], {}
    for pos in np.ndindex(grid, grid, grid):
        data = first if not sims else DeviceArray.empty((n, n, n), np.uint16)
        if sims:
            first.copy_into(data, (0, 0, 0))
        affine = np.eye(4)
        affine[:3, 3] = [p * step for p in pos]
        index[pos] = len(sims)
        sim = si.to_spatial_image(data, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0,) * 3)), translation=dict(zip("zyx", (0.0,) * 3)))
        si.set_sim_affine(sim, affine, transform_key="stage")
        sims.append(sim)
    pairs = [(index[pos], index[pos[:ax] + (pos[ax] + 1,) + pos[ax + 1:]]) for pos in index for ax in range(3) if pos[ax] + 1 < grid]
    _lib.synchronize(0)
    spent = {"moments": 0.0, "solve": 0.0}
    real_moments, real_solve = _intensity_ops.cell_pair_moments, intensity.solve_maps

    def timed(key, fn):
        def wrapper(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                spent[key] += time.perf_counter() - t0
        return wrapper

    _intensity_ops.cell_pair_moments = timed("moments", real_moments)
    intensity.solve_maps = timed("solve", real_solve)
    try:
        for cells in (1, 4):
            for attempt in ("first call", "second call"):
                spent.update(moments=0.0, solve=0.0)
                t0 = time.perf_counter()
                maps, info = intensity.fit_maps(sims, "stage", cells=cells, pairs=pairs, return_info=True)
                wall = time.perf_counter() - t0
                lines.append(f"fit_maps, {len(sims)} tiles of {n}^3 uint16, {len(pairs)} pairs, cells={cells} ({attempt}): wall {wall:.3f} s = "
                             f"moment kernels {spent['moments']:.3f} s + solve {spent['solve']:.3f} s + geometry and planning "
                             f"{wall - spent['moments'] - spent['solve']:.3f} s; N = {info['N']:.0f} sample pairs")
    finally:
        _intensity_ops.cell_pair_moments, intensity.solve_maps = real_moments, real_solve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--grid", type=int, default=4)
    ap.add_argument("--skip-fit", action="store_true")
    args = ap.parse_args()
    _lib.init(0)
    lines = []
    apply_leg(args.tile, lines)
    if not args.skip_fit:
        fit_leg(args.tile, args.grid, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
