"""Bead detection on one 512^3 uint16 tile resident in HBM (about 2000 beads of 6 voxels, default parameters).
Prints one JSON line: wall ms of one mvs_log_response and one mvs_local_maxima call (each launched twice, the second one timed;
both wait for their result), the HBM bytes their passes move per voxel and the share of 8 TB/s that makes, the wall time of
detect_beads on the resident tile, the number of points, and -- for scale -- the wall time of the scipy restatement
(tests/detection_oracle.py) on a 128^3 crop of the same tile.  Every step runs under a time limit: a call that does not return
ends the probe.

    python tools/detect_probe.py [--size 512] [--limit 120]
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

HBM_PEAK = 8.0e12           # B/s
DIAMETER = 6.0
# HBM bytes per voxel and pass (uint16 tile): x reads 2, writes 8; y reads 8, writes 8; z reads 8, writes 4
LOG_BYTES = (2 + 8) + (8 + 8) + (8 + 4)
# running maximum along x and y: 4 + 4 each; last pass reads the response and the running maximum
MAXIMA_BYTES = 8 + 8 + 8


class _Limit:
    """SIGALRM after ``seconds``: the default action ends the process."""

    def __init__(self, seconds):
        self.seconds = int(seconds)

    def __enter__(self):
        signal.signal(signal.SIGALRM, signal.SIG_DFL)
        signal.alarm(self.seconds)

    def __exit__(self, *exc):
        signal.alarm(0)


def _second_call_ms(fn, limit):
    with _Limit(limit):
        fn()
        t = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t) * 1e3, out


def make_tile(size, n_beads, seed=0):
    """Background 100 + noise of sigma 8, beads of amplitude 2000..4000 and sigma DIAMETER / (2 sqrt 3) added as small patches."""
    rng = np.random.default_rng(seed)
    tile = rng.normal(100.0, 8.0, (size,) * 3).astype(np.float32)
    sig = DIAMETER / (2.0 * np.sqrt(3.0))
    h = 7
    g = np.arange(-h, h + 1, dtype=np.float64)
    cell = int(2.5 * DIAMETER)
    cells = rng.permutation((size // cell) ** 3)[:n_beads]
    per = size // cell
    for cidx in cells:
        c = np.array(np.unravel_index(cidx, (per,) * 3)) * cell + cell // 2
        c = np.clip(c, h, size - h - 1)
        off = rng.uniform(-0.35, 0.35, 3)
        patch = rng.uniform(2000.0, 4000.0) * np.exp(-0.5 * (((g - off[0]) / sig) ** 2)[:, None, None]
                                                     - 0.5 * (((g - off[1]) / sig) ** 2)[None, :, None]
                                                     - 0.5 * (((g - off[2]) / sig) ** 2)[None, None, :])
        tile[tuple(slice(int(k) - h, int(k) + h + 1) for k in c)] += patch.astype(np.float32)
    return np.clip(np.rint(tile), 0, 65535).astype(np.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--beads", type=int, default=2000)
    ap.add_argument("--limit", type=int, default=120, help="seconds for each step")
    a = ap.parse_args()

    from multiview_stitcher_amd import _detect_ops, _lib, detection, msi_utils
    from multiview_stitcher_amd import spatial_image_utils as si
    from multiview_stitcher_amd.device import DeviceArray
    from tests import detection_oracle as do

    dev = 0
    _lib.init(dev)
    tile = make_tile(a.size, a.beads)
    n = float(tile.size)
    spacing = (1.0, 1.0, 1.0)
    sigma, _, window = detection.log_detect_parameters(spacing, DIAMETER)
    res = {"shape": list(tile.shape), "dtype": "uint16", "sigma": sigma[0], "radius": int(4 * sigma[0] + 0.5), "window": window[0]}
    with _Limit(a.limit):
        d_tile = DeviceArray.from_host(tile, dev)

    ms, (response, peak) = _second_call_ms(lambda: _detect_ops.log_response(d_tile, sigma, float(np.mean(sigma)) ** 2, device=dev), a.limit)
    res["log_response_ms"] = ms
    res["log_response_bytes_per_voxel"] = LOG_BYTES
    res["log_response_frac_of_hbm_peak"] = LOG_BYTES * n / (ms * 1e-3) / HBM_PEAK
    threshold = np.float32(peak) * 0.2
    ms, coords = _second_call_ms(lambda: _detect_ops.local_maxima(response, window, threshold, device=dev), a.limit)
    res["local_maxima_ms"] = ms
    res["local_maxima_bytes_per_voxel"] = MAXIMA_BYTES
    res["local_maxima_frac_of_hbm_peak"] = MAXIMA_BYTES * n / (ms * 1e-3) / HBM_PEAK
    res["detected_voxels"] = int(len(coords))
    del response

    sim = si.to_spatial_image(d_tile, dims=["z", "y", "x"], scale=dict(zip("zyx", spacing)), translation=dict(zip("zyx", (0.0, 0.0, 0.0))))
    msim = msi_utils.get_msim_from_sim(sim)
    ms, points = _second_call_ms(lambda: detection.detect_beads(msim, detection_func_kwargs={"target_size_physical": DIAMETER}, device=dev), a.limit)
    res["detect_beads_ms"] = ms
    res["points"] = int(len(points))

    crop = np.ascontiguousarray(tile[:128, :128, :128])
    with _Limit(a.limit):
        t = time.perf_counter()
        labels = do.log_detect(crop, spacing, DIAMETER)
        do.label_centroids(labels)
        res["oracle_128_cube_s"] = time.perf_counter() - t
    res["oracle_scaled_to_tile_s"] = res["oracle_128_cube_s"] * n / crop.size
    print(json.dumps(res))


if __name__ == "__main__":
    main()
