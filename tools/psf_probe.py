"""PSF extraction from beads, timed: mvs_psf_extract (through _psf_ops.psf_extract) over N beads with a W^3 window on an S^3 uint16
tile resident on the device, against the numpy / scipy restatement (tests/psf_oracle.py) on the host for a bounded sample of the
same beads, extrapolated linearly to N (the restatement's cost is per bead).

Device figures: the HIP-event time of the call's launch chain (mvs_last_kernel_ms: events around the kernels, including the one
host wait between the average and the correlations) and the wall time, both of the SECOND of two calls.  The restatement runs
on a crop of the tile that holds the sampled beads' windows (its float64 copy of a whole 512^3 tile would be 1 GiB), in one
process.

    python tools/psf_probe.py [--beads 2048] [--window 31] [--size 512] [--sample 27] [--out profiles/psf_extract.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_tile(size, n_beads, pitch, rng):
    """uint16 tile: background 100, Gaussian beads of sigma (2.0, 1.2, 1.5) stamped on a lattice of `pitch`, jittered by half a pixel."""
    per_axis = int(np.ceil(n_beads ** (1.0 / 3.0)))
    first = pitch // 2 + 4
    assert first + pitch * (per_axis - 1) + pitch // 2 + 4 < size, "the lattice does not fit the tile"
    lattice = np.array([(z, y, x) for z in range(per_axis) for y in range(per_axis) for x in range(per_axis)][:n_beads], dtype=np.float64)
    truth = first + pitch * lattice + rng.uniform(-0.5, 0.5, lattice.shape)
    amp = rng.uniform(500.0, 3000.0, n_beads)
    tile = np.full((size,) * 3, 100.0, dtype=np.float32)
    half = 10
    grid = np.arange(-half, half + 1, dtype=np.float64)
    for p, a in zip(truth, amp):
        c = np.rint(p).astype(int)
        d = [grid + ci - pi for ci, pi in zip(c, p)]
        stamp = a * np.exp(-(d[0][:, None, None] ** 2 / 8.0 + d[1][None, :, None] ** 2 / 2.88 + d[2][None, None, :] ** 2 / 4.5))
        tile[tuple(slice(ci - half, ci + half + 1) for ci in c)] += stamp.astype(np.float32)
    return np.rint(tile).astype(np.uint16), truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--beads", type=int, default=2048)
    ap.add_argument("--window", type=int, default=31)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sample", type=int, default=27)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from multiview_stitcher_amd import _lib, _psf_ops
    from multiview_stitcher_amd.device import DeviceArray
    from tests import psf_oracle as po

    r = (args.window - 1) // 2
    radius = (r, r, r)
    tile, truth = make_tile(args.size, args.beads, args.window + 5, np.random.default_rng(1))
    given = np.rint(truth)
    lines = [f"psf_probe: {args.beads} beads, window {args.window}^3, tile {args.size}^3 uint16 (device-resident), 1 refinement"]

    dev = DeviceArray.from_host(tile, args.device)
    res = None
    for _ in range(2):
        t = time.perf_counter()
        res = _psf_ops.psf_extract(dev, given, np.eye(3), radius, 1, args.device)
        wall = (time.perf_counter() - t) * 1e3
        kernel = _lib.last_kernel_ms(args.device)
    psf, centers, status, stats = res
    lines.append(f"device: launch chain {kernel:.3f} ms (HIP events), call {wall:.3f} ms wall; {int((status == 0).sum())} beads used, "
                 f"refined centres within {np.abs(centers - truth)[status == 0].max():.4f} px of the truth, min ncc {np.nanmin(stats[:, 2]):.4f}")

    # the restatement on up to `sample` beads whose windows share one corner crop of the tile
    cells = int(np.ceil(args.sample ** (1.0 / 3.0)))
    hi = min(int(given.min()) + (cells - 1) * (args.window + 5) + r + 3, args.size)
    inside = np.nonzero(np.all(given + r + 1 < hi, axis=1))[0][: args.sample]
    crop = np.ascontiguousarray(tile[:hi, :hi, :hi])
    t = time.perf_counter()
    want = po.extract(crop, given[inside], np.eye(3), radius, 1)
    host = (time.perf_counter() - t) * 1e3
    lines.append(f"restatement (numpy / scipy, one process): {host:.1f} ms for {len(inside)} beads on a {hi}^3 crop = {host / len(inside):.2f} ms per bead, "
                 f"{host / len(inside) * args.beads:.0f} ms extrapolated to {args.beads} beads (the average over another bead set: not compared)")
    lines.append(f"agreement on the sampled beads: centres {np.abs(want['centers'] - centers[inside]).max():.2e} px")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
