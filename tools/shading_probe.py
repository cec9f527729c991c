"""Measurements of the shading correction on one GPU:

  1. mvs_plane_apply on one resident 512^3 uint16 tile -- out of place, in place, uint16 -> float32 -- against mvs_intensity_apply
     and a device-to-device copy of the same bytes, in the same process and in alternating rounds (warm-up, medians, spread);
  2. mvs_stack_quantiles on the north-star stack (64 resident tiles of 512^3 uint16), q = 0.5 and (0.02, 0.5): wall and kernel
     time, GB/s of the bytes the algorithm reads (stack bytes times 1 + n_q * (digits - 1) passes), next to the copy above;
  3. np.quantile(method="lower") of a sub-stack on the host, scaled to the whole stack;
  4. intensity.estimate_shading end to end on that stack: device time against host time.

    python tools/shading_probe.py --out profiles/shading_probe.txt [--tile 512] [--tiles 64] [--host-planes 4]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _intensity_ops, _lib, _shading_ops, intensity  # noqa: E402
from multiview_stitcher_amd import spatial_image_utils as si  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402


def timed_ms(fn):
    _lib.synchronize(0)
    t0 = time.perf_counter()
    fn()
    _lib.synchronize(0)
    return (time.perf_counter() - t0) * 1e3


def alternating(legs, warmup=3, rounds=10):
    """Every leg once per round, the rounds in turn: {name: (median, min, max, last kernel ms)} in ms."""
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    times = {name: [] for name in legs}
    kernel = {}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(timed_ms(fn))
            kernel[name] = _lib.last_kernel_ms(0)
    return {name: (statistics.median(t), min(t), max(t), kernel[name]) for name, t in times.items()}


def apply_leg(n, lines):
    rng = np.random.default_rng(0)
    tile = DeviceArray.from_host(rng.integers(0, 60000, size=(n, n, n), dtype=np.uint16))
    out = DeviceArray.empty((n, n, n), np.uint16)
    out32 = DeviceArray.empty((n, n, n), np.float32)
    cells = np.stack([rng.random((4, 4, 4)) * 0.2 + 0.9, rng.random((4, 4, 4)) * 50], axis=-1).astype(np.float32)
    plane = DeviceArray.from_host(np.stack([rng.random((n, n)) * 0.2 + 0.9, rng.random((n, n)) * 50], axis=-1).astype(np.float32))
    legs = {
        "device-to-device copy": lambda: tile.copy_into(out, (0, 0, 0)),
        "intensity_apply, out of place": lambda: _intensity_ops.apply_map(tile, cells, out=out),
        "plane_apply, out of place": lambda: _shading_ops.apply_plane(tile, plane, out=out),
        "intensity_apply, in place": lambda: _intensity_ops.apply_map(tile, cells, out=tile),
        "plane_apply, in place": lambda: _shading_ops.apply_plane(tile, plane, out=tile),
        "intensity_apply, uint16 -> float32": lambda: _intensity_ops.apply_map(tile, cells, out=out32, out_dtype=np.float32),
        "plane_apply, uint16 -> float32": lambda: _shading_ops.apply_plane(tile, plane, out=out32, out_dtype=np.float32),
    }
    res = alternating(legs)
    for name, (med, lo, hi, kern) in res.items():
        moved = (tile.nbytes + (out32.nbytes if "float32" in name else tile.nbytes)) / 1e9
        kernel = f", kernel {kern:.3f} ms" if "apply" in name else ""
        lines.append(f"{name:36s} {n}^3 uint16: median {med:.3f} ms (min {lo:.3f}, max {hi:.3f}) of 10 alternating rounds after 3 warm-up rounds, "
                     f"{moved:.3f} GB read + written -> {moved / med * 1e3:.0f} GB/s{kernel}")
    for variant in ("out of place", "in place", "uint16 -> float32"):
        a, b = res[f"plane_apply, {variant}"][0], res[f"intensity_apply, {variant}"][0]
        lines.append(f"plane_apply / intensity_apply, {variant}: {a / b:.3f} (the margin is 1.10)")
    return res["device-to-device copy"][0], 2 * tile.nbytes / 1e9


def stack_leg(n, n_tiles, host_planes, copy_ms, copy_gb, lines):
    rng = np.random.default_rng(1)
    base = [rng.integers(0, 60000, size=(n, n, n), dtype=np.uint16) for _ in range(2)]
    tiles = [DeviceArray.from_host(base[v % 2] ^ np.uint16(37 * v)) for v in range(n_tiles)]
    stack_gb = sum(t.nbytes for t in tiles) / 1e9
    _lib.synchronize(0)
    for q in ([0.5], [0.02, 0.5]):
        passes = 1 + len(q) * (tiles[0].dtype.itemsize - 1)
        res = alternating({"q": lambda q=q: _shading_ops.stack_quantiles(tiles, q)}, warmup=1, rounds=5)["q"]
        med, lo, hi, kern = res
        lines.append(f"stack_quantiles, {n_tiles} resident tiles of {n}^3 uint16 ({stack_gb:.1f} GB), q = {q}: median {med:.1f} ms (min {lo:.1f}, max {hi:.1f}) "
                     f"of 5 after 1 warm-up call, kernel {kern:.1f} ms; {passes} passes = {passes * stack_gb:.1f} GB read -> "
                     f"{passes * stack_gb / kern * 1e3:.0f} GB/s in the kernel; the copy of one tile in this process moves {copy_gb / copy_ms * 1e3:.0f} GB/s "
                     f"(read + written), so the kernel reads at {passes * stack_gb / kern / (copy_gb / copy_ms):.2f} of the copy's rate")
    # the host: numpy's own quantile of host_planes planes of every tile
    sub = np.concatenate([base[v % 2][:host_planes] ^ np.uint16(37 * v) for v in range(n_tiles)], axis=0)
    t0 = time.perf_counter()
    want = np.quantile(sub, 0.5, axis=0, method="lower")
    host_s = time.perf_counter() - t0
    got, _ = _shading_ops.stack_quantiles([t[:host_planes] for t in tiles], 0.5)
    assert np.array_equal(got[0], want.astype(np.float32))
    lines.append(f"np.quantile(method='lower') of {sub.shape[0]} planes of {n}^2 uint16 ({sub.nbytes / 1e9:.2f} GB) on the host: {host_s:.2f} s, equal to the "
                 f"device's planes; scaled to the {n_tiles * n} planes of the stack: {host_s * n_tiles * n / sub.shape[0]:.0f} s")
    # end to end
    sims = [si.to_spatial_image(t, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0,) * 3)), translation=dict(zip("zyx", (0.0,) * 3))) for t in tiles]
    spent = {"device": 0.0}
    real = _shading_ops.stack_quantiles

    def timed(*a, **k):
        t0 = time.perf_counter()
        try:
            return real(*a, **k)
        finally:
            spent["device"] += time.perf_counter() - t0

    _shading_ops.stack_quantiles = timed
    try:
        for attempt in ("first call", "second call"):
            spent["device"] = 0.0
            t0 = time.perf_counter()
            intensity.estimate_shading(sims)
            wall = time.perf_counter() - t0
            lines.append(f"estimate_shading, {n_tiles} tiles of {n}^3 uint16, degree 4 ({attempt}): wall {wall:.3f} s = stack_quantiles {spent['device']:.3f} s "
                         f"+ host fit {wall - spent['device']:.3f} s")
    finally:
        _shading_ops.stack_quantiles = real


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--host-planes", type=int, default=4)
    args = ap.parse_args()
    _lib.init(0)
    lines = []
    copy_ms, copy_gb = apply_leg(args.tile, lines)
    stack_leg(args.tile, args.tiles, args.host_planes, copy_ms, copy_gb, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
