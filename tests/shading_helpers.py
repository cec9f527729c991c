"""Shared by tests/test_shading_host.py and tests/test_shading_gpu.py: the planted shading profile, the two end-to-end cases built
on it, and their oracle planes, computed once."""
import functools

import numpy as np
from scipy import ndimage

from tests import shading_oracle as so
from tests.metrics_helpers import make_tile, translation_affine

RECOVERY_CAP = 0.05               # max |F / F0 - 1| of a recovered flat field: a condition of the tests, not a measurement
U16_SCALE = 10000.0               # counts per unit of the float32 tiles in the uint16 variants
# (tiles, tile shape).  With 6 and 36 tiles the oracle's planes gave max |F / F0 - 1| of 0.020 .. 0.053 and 0.022 .. 0.047 over three
# seeds -- the noise of the per-pixel median at the corners of the fit; four times the tiles halve it: 0.015 .. 0.022 and
# 0.006 .. 0.025 over four seeds (seed 0, the one the tests use: 0.0156 and 0.0118).
CASES = {"stack3d": (24, (24, 64, 64)), "tiles2d": (144, (96, 96))}


def planted_flat(h, w):
    """F0 = 1 - 0.25 (y - 0.1)^2 - 0.15 (x + 0.05)^2 + 0.04 x y on [-1, 1]^2, scaled to mean 1: up to 43 % from 1."""
    y, x = np.meshgrid(np.linspace(-1, 1, h), np.linspace(-1, 1, w), indexing="ij")
    f = 1.0 - 0.25 * (y - 0.1) ** 2 - 0.15 * (x + 0.05) ** 2 + 0.04 * x * y
    return f / f.mean()


def planted_dark(h, w):
    """D0 = 0.1 + 0.02 y."""
    y = np.linspace(-1, 1, h)[:, None]
    return np.broadcast_to(0.1 + 0.02 * y, (h, w)).copy()


def field(shape, seed):
    """A field like intensity_helpers.texture's float32 one: smoothed noise stretched to [0.5, 3.5]."""
    rng = np.random.default_rng(seed)
    t = ndimage.gaussian_filter(rng.random(shape), 1.2)
    return (t - t.min()) / (t.max() - t.min()) * 3.0 + 0.5


@functools.lru_cache(maxsize=None)
def planted_case(name, dtype_name, seed=0):
    """Independent fields S_v seen through the planted profile: tile v stores F0 * S_v + D0 (uint16: times U16_SCALE, rounded).
    Returns the tiles, their msims, F0, the dark field in the tiles' units, and the clean tiles S_v + mean(D0) in those units."""
    n, shape = CASES[name]
    h, w = shape[-2:]
    f0, d0 = planted_flat(h, w), planted_dark(h, w)
    scale = U16_SCALE if dtype_name == "u16" else 1.0
    dtype = np.uint16 if dtype_name == "u16" else np.float32
    tiles, clean = [], []
    for v in range(n):
        s = field(shape, 1000 * seed + 17 * v + 3)
        raw = (f0 * s + d0) * scale
        tiles.append(np.rint(raw).astype(dtype) if dtype_name == "u16" else raw.astype(dtype))
        clean.append((s + d0.mean()) * scale)
    aff = {"stage": translation_affine([0.0] * len(shape))}
    msims = [make_tile(t, aff)[0] for t in tiles]
    return {"tiles": tiles, "msims": msims, "flat": f0, "dark": d0 * scale, "clean": clean, "scale": scale}


@functools.lru_cache(maxsize=None)
def oracle_planes(name, dtype_name, seed=0):
    """Median plane and counts of a planted case by sorting."""
    return so.stack_quantiles(planted_case(name, dtype_name, seed)["tiles"], [0.5])


def recovery_error(shading, case):
    return float(np.abs(shading["flatfield"].astype(np.float64) / case["flat"] - 1.0).max())
