"""Cost of label stitching at size: two resident (512, 512, 512) int32 label tiles with 110 voxels of overlap
along x and about 10^5 labels each (blocks of 11^3 voxels of one world-wide block grid, renumbered at random per tile), REPS times
each after a warm-up:

  counts   mvs_label_counts of one tile, the capacity sized beforehand (one call)
  pairs    mvs_label_pair_overlaps of the pair at a capacity of 2^16 triples (a table of 2^17 slots); prints the table's occupancy
  fuse     mvs_label_tiles_fuse of both tiles through the tables of labels.match_labels onto the whole (512, 512, 914) grid, the
           result left on the device
  masks    mvs_label_fuse of two resident uint8 masks of the same geometry onto the same grid: the same access pattern without the
           table gather, for comparison

    python tools/labels_probe.py [REPS]

Prints the event-timed milliseconds (``_lib.last_kernel_ms``) and the wall milliseconds of every call; draws no bar from them."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _label_ops, _lib, _mask_ops, labels  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
DEVICE = 0
N, OVERLAP, BLOCK = 512, 110, 11


def block_labels(x0, seed):
    """The tile at world x0: the world's block ids (1-based), renumbered by a random permutation of the tile's own."""
    per = -(-(2 * N) // BLOCK)
    zy = (np.arange(N) // BLOCK).astype(np.int32)
    x = ((np.arange(N) + x0) // BLOCK).astype(np.int32)
    ids = (zy[:, None, None] * per + zy[None, :, None]) * per + x[None, None, :]
    present = np.zeros(per ** 3, dtype=bool)
    present[(zy[:, None, None] * per + zy[None, :, None]) * per + np.unique(x)[None, None, :]] = True
    new = np.zeros(per ** 3, dtype=np.int32)
    new[present] = np.random.default_rng(seed).permutation(int(present.sum())).astype(np.int32) + 1
    return new[ids]


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
    x0 = N - OVERLAP
    host = [block_labels(0, 1), block_labels(x0, 2)]
    tiles = [_label_ops.to_device(t, DEVICE) for t in host]
    n_labels = [int(t.max()) for t in host]
    print(f"tiles {host[0].shape} int32, {n_labels} labels, overlap {OVERLAP} voxels along x")
    del host
    matrix, offset = np.eye(3), np.array([0.0, 0.0, -float(x0)])
    box_lo, box_n = labels.footprint_box(matrix, offset, (N, N, N), (N, N, N))

    cap = 1 << 17
    counts = [_label_ops.label_counts(t, DEVICE, capacity=cap) for t in tiles]
    assert all(int(c.sum()) == N ** 3 for c in counts)
    timed("counts", lambda: _label_ops.label_counts(tiles[0], DEVICE, capacity=cap), f" -> {4 * N ** 3 / 1e9:.2f} GB read")

    table = _label_ops.pair_overlaps(tiles[0], tiles[1], matrix, offset, box_lo, box_n, DEVICE, capacity=1 << 16)
    assert int(table[2].sum()) == N * N * OVERLAP
    slots = 1 << 17
    timed("pairs", lambda: _label_ops.pair_overlaps(tiles[0], tiles[1], matrix, offset, box_lo, box_n, DEVICE, capacity=1 << 16),
          f" -> {len(table[0])} entries in {slots} slots: occupancy {len(table[0]) / slots:.3f}; box {box_n}")

    luts, n_objects = labels.match_labels(counts, {(0, 1): table})
    print(f"match_labels: {n_objects} objects of {sum(n_labels)} labels")
    out_shape = (N, N, N + x0)
    matrices, offsets = [np.eye(3), np.eye(3)], [np.zeros(3), offset]
    fused = _label_ops.fuse_label_tiles(tiles, matrices, offsets, luts, out_shape, None, DEVICE, out_on_device=True)
    assert fused.shape == out_shape
    del fused
    ms_fuse = timed("fuse", lambda: _label_ops.fuse_label_tiles(tiles, matrices, offsets, luts, out_shape, None, DEVICE, out_on_device=True),
                    f" -> {int(np.prod(out_shape))} output voxels")
    ms_ident = timed("fuse, identity tables", lambda: _label_ops.fuse_label_tiles(tiles, matrices, offsets, None, out_shape, None, DEVICE, out_on_device=True))

    masks = [DeviceArray.from_host(np.ones((N, N, N), np.uint8), DEVICE) for _ in range(2)]
    ms_masks = timed("masks (mvs_label_fuse)", lambda: _mask_ops.fuse_labels(masks, matrices, offsets, out_shape, DEVICE, out_on_device=True))
    print(f"fuse / masks (medians): {ms_fuse / ms_masks:.3f}; identity / masks: {ms_ident / ms_masks:.3f}")


if __name__ == "__main__":
    main()
