"""Cost of connected-component labelling at size (DESIGN.md, section on mvs_label_components): one resident (512, 512, 512) uint16
tile of blobs -- Gaussian-filtered noise, so objects of every size with ragged surfaces -- thresholded at its Otsu level
(``masks.otsu_threshold``), labelled at connectivity 1 and 3, REPS times each after a warm-up, the result left on the device:

  labels     mvs_label_components, every component kept (six launches)
  filtered   the same with min_voxels = 20 (the flatten launch also counts the voxels per root)
  scipy      scipy.ndimage.label of the same mask on this machine's CPU: the time to compare with (one run)

    python tools/components_probe.py [REPS] [N] [ONLY]

ONLY: ``c1`` / ``c3`` (labels at that connectivity alone) or ``c1f`` / ``c3f`` (filtered alone), for a kernel trace of one variant.

Prints the event-timed milliseconds of the chain (``_lib.last_kernel_ms``) and the wall milliseconds of the call, the bytes the
launches stream by their own arithmetic (chases and gathers not counted) against the minimum of 2 + 4 bytes per voxel, and checks
the result against scipy's.  The share of each launch comes from a kernel trace of this same command:

    bash tools/kprofile.sh -o components_probe -k "component_" -- python tools/components_probe.py 5 512 c1

Draws no bar from any of it."""
import os
import sys
import time

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _label_ops, _lib, masks  # noqa: E402
from multiview_stitcher_amd import spatial_image_utils as si  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 512
ONLY = sys.argv[3] if len(sys.argv) > 3 else ""
DEVICE = 0


def blobs(n, seed=0):
    """uint16 blobs: noise filtered with sigma 3, stretched to 0 .. 60000."""
    f = ndimage.gaussian_filter(np.random.default_rng(seed).random((n, n, n), dtype=np.float32), 3.0)
    f -= f.min()
    return (f * (60000.0 / f.max())).astype(np.uint16)


def timed(name, call, note=""):
    call()
    ev, wall = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        _lib.synchronize(DEVICE)
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(_lib.last_kernel_ms(DEVICE))
    ev, wall = np.array(ev), np.array(wall)
    print(f"{name}: event ms median {np.median(ev):.3f} min {ev.min():.3f} max {ev.max():.3f}; wall ms median {np.median(wall):.3f} ({REPS} runs){note}")
    return float(np.median(ev))


def main():
    _lib.init(DEVICE)
    host = blobs(N)
    sim = si.to_spatial_image(host, dims=["z", "y", "x"], scale=dict(zip("zyx", (1.0,) * 3)), translation=dict(zip("zyx", (0.0,) * 3)))
    threshold = float(masks.otsu_threshold([sim], device=DEVICE))
    tile = DeviceArray.from_host(host, DEVICE)
    voxels = host.size
    mask = host.astype(np.float32) > np.float32(threshold)
    print(f"tile {host.shape} uint16, Otsu threshold {threshold:.1f}, foreground {mask.mean():.3f} of {voxels} voxels")
    minimum = 6 * voxels
    # rows: read 2, write 4; merge: the rows' parents again (4) and the neighbour rows through the caches; flatten: read 4 (writes only
    # where a voxel was no child of its root yet); count and rank: read 4 each; relabel: read 4, write 4.  Sizes: one atomic per run.
    streamed = (2 + 4 + 4 + 4 + 4 + 4 + 4 + 4) * voxels
    print(f"streamed by the launches' own arithmetic: {streamed / 1e9:.2f} GB = {streamed / minimum:.1f} x the minimum of {minimum / 1e9:.2f} GB (2 + 4 bytes per voxel)")
    for connectivity in (1, 3):
        if ONLY and ONLY[:2] != f"c{connectivity}":
            continue
        t0 = time.perf_counter()
        want, want_n = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, connectivity))
        cpu_ms = (time.perf_counter() - t0) * 1e3
        got, n = _label_ops.label_components(tile, threshold, connectivity=connectivity, device=DEVICE)
        assert n == want_n and np.array_equal(got.get(), want), "the labels differ from scipy's"
        sizes = np.bincount(want.ravel())[1:]
        print(f"connectivity {connectivity}: {n} components, the largest {int(sizes.max())} voxels, {int((sizes < 20).sum())} below 20 voxels; "
              f"scipy.ndimage.label {cpu_ms:.0f} ms on {os.cpu_count()} CPUs (one thread)")
        del want, got
        if ONLY.endswith("f"):
            timed(f"filtered c{connectivity}", lambda: _label_ops.label_components(tile, threshold, connectivity=connectivity, min_voxels=20, device=DEVICE))
            continue
        ms = timed(f"labels   c{connectivity}", lambda: _label_ops.label_components(tile, threshold, connectivity=connectivity, device=DEVICE))
        print(f"    -> {minimum / ms / 1e6:.0f} GB/s of the minimum, {streamed / ms / 1e6:.0f} GB/s of the streamed bytes; scipy / GPU = {cpu_ms / ms:.0f}")
        if not ONLY:
            timed(f"filtered c{connectivity}", lambda: _label_ops.label_components(tile, threshold, connectivity=connectivity, min_voxels=20, device=DEVICE))


if __name__ == "__main__":
    main()
