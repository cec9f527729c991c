"""Cost of masks as fusion weights, for tools/kprofile.sh:

  fuse    one resident 3-D chunk -- 2 x 2 tiles of (128, 512, 512) uint16 with 64 voxels of overlap, the result left on the device --
          through mvs_fuse_chunk_weighted with all-252 tiles and through mvs_fuse_chunk under option "force_generic", alternating,
          REPS times each after a warm-up of both; the two results must have equal bytes
  feather mvs_mask_feather of a resident 256^3 blob mask at widths 4 and 32, REPS times each after a warm-up

    bash tools/kprofile.sh -o view_weights -k "fuse_weighted_kernel|fuse_kernel|feather" -- python tools/view_weights_probe.py [REPS]

Prints the event-timed milliseconds of every call (``_lib.last_kernel_ms``); the kernel statistics come from the trace."""
import os
import sys

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from multiview_stitcher_amd import _lib, _mask_ops, fusion  # noqa: E402
from multiview_stitcher_amd import device as dev_mod  # noqa: E402
from multiview_stitcher_amd import spatial_image_utils as si  # noqa: E402
from multiview_stitcher_amd.device import DeviceArray  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
DEVICE = 0
SD = ["z", "y", "x"]


def fuse_part():
    shape, step = (128, 512, 512), (0, 448, 448)
    rng = np.random.default_rng(0)
    sims, tiles, params = [], [], []
    for iy in range(2):
        for ix in range(2):
            origin = dict(zip(SD, (0.0, float(iy * step[1]), float(ix * step[2]))))
            data = rng.integers(0, 65536, size=shape, dtype=np.uint16)
            sims.append(dev_mod.to_device(si.to_spatial_image(data, dims=SD, scale=dict(zip(SD, (1.0, 1.0, 1.0))), translation=origin), DEVICE))
            tiles.append(DeviceArray.from_host(np.full(shape, 252, np.uint8), DEVICE))
            params.append(np.eye(4))
    out_shape = (shape[0], shape[1] + step[1], shape[2] + step[2])
    box = {"origin": dict(zip(SD, (0.0, 0.0, 0.0))), "spacing": dict(zip(SD, (1.0, 1.0, 1.0))), "shape": dict(zip(SD, out_shape))}
    outs = [DeviceArray.empty(out_shape, np.uint16, DEVICE) for _ in range(2)]

    def weighted():
        fusion.fuse_np(sims, params, box, out=outs[0], view_weights=tiles, device=DEVICE)
        _lib.synchronize(DEVICE)
        return _lib.last_kernel_ms(DEVICE)

    def generic():
        _lib.set_option("force_generic", 1, DEVICE)
        try:
            fusion.fuse_np(sims, params, box, out=outs[1], device=DEVICE)
        finally:
            _lib.set_option("force_generic", 0, DEVICE)
        _lib.synchronize(DEVICE)
        return _lib.last_kernel_ms(DEVICE)

    weighted(), generic()
    ms = {"weighted": [], "generic": []}
    for _ in range(REPS):
        ms["weighted"].append(weighted())
        ms["generic"].append(generic())
    same = np.array_equal(outs[0].get(), outs[1].get())
    n_out = int(np.prod(out_shape))
    for key, v in ms.items():
        v = np.array(v)
        print(f"fuse {key}: {n_out} output voxels, event ms median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} ({REPS} runs)")
    print(f"fuse ratio weighted / generic (medians): {np.median(ms['weighted']) / np.median(ms['generic']):.3f}; equal bytes: {same}")
    assert same


def feather_part():
    shape = (256, 256, 256)
    field = ndimage.gaussian_filter(np.random.default_rng(7).random(shape, dtype=np.float32), 6.0, mode="nearest")
    mask = DeviceArray.from_host((field > np.quantile(field, 0.35)).astype(np.uint8), DEVICE)
    for width in (4, 32):
        _mask_ops.feather(mask, width, DEVICE, out_on_device=True)
        v = []
        for _ in range(REPS):
            _mask_ops.feather(mask, width, DEVICE, out_on_device=True)
            v.append(_lib.last_kernel_ms(DEVICE))
        v = np.array(v)
        must = 2 * int(np.prod(shape))      # the mask read once, the tile written once
        print(f"feather width {width}: {must / 1e6:.1f} MB to move, event ms median {np.median(v):.3f} min {v.min():.3f} max {v.max():.3f} "
              f"({REPS} runs) -> {must / np.median(v) / 1e6:.1f} GB/s of that")


if __name__ == "__main__":
    _lib.init(DEVICE)
    fuse_part()
    feather_part()
