"""Weight tiles for the cases of tests/affine_cases.py (tests/test_fuse_weights_host.py, tests/test_fuse_weighted_gpu.py): per view a
smooth random blob mask (tests/mask_feather_cases.py) feathered by the scipy oracle of ``masks.feather``, in the two forms the
tests need -- the oracle's ``{"data", "origin", "spacing"}`` and a sim for the library."""
import functools

import numpy as np

from tests import affine_cases as ac
from tests import mask_feather_cases as fc
from tests import mask_feather_oracle as feather_oracle
from tests.helpers import sim_to_view

WIDTHS = {2: (6, 9), 3: (2, 6, 9)}


def tile_sim(data, like, origin=None, spacing=None):
    """A weight tile as a sim on the grid of ``like`` (or on ``origin`` / ``spacing`` given per dim), without transforms."""
    from multiview_stitcher_amd import spatial_image_utils as si

    sdims = si.get_spatial_dims_from_sim(like)
    origin = si.get_origin_from_sim(like) if origin is None else origin
    spacing = si.get_spacing_from_sim(like) if spacing is None else spacing
    return si.to_spatial_image(np.asarray(data), dims=sdims, scale={d: float(spacing[d]) for d in sdims}, translation={d: float(origin[d]) for d in sdims})


def as_oracle_tile(sim):
    if sim is None:
        return None
    view, _ = sim_to_view(sim)
    return view


@functools.lru_cache(maxsize=None)
def _tiles(name, dtype, background):
    sims = ac.build(name, dtype)[0]
    out = []
    for i, s in enumerate(sims):
        shape = tuple(int(n) for n in s.data.shape)
        mask = fc.blob_mask(shape, seed=100 + i, background=background, sigma=3.0)
        w = feather_oracle.feather(mask, WIDTHS[len(shape)])
        w.setflags(write=False)
        out.append(w)
    return tuple(out)


def feathered_tiles(name, dtype=np.uint16, background=0.35):
    """Per view of case ``name`` its feathered uint8 tile on the view's own grid (a tuple of read-only arrays, built once)."""
    return _tiles(name, np.dtype(dtype), background)


def masks_of(name, dtype=np.uint16, background=0.35):
    """The blob masks ``feathered_tiles`` feathers, in the same order."""
    return [fc.blob_mask(tuple(int(n) for n in s.data.shape), seed=100 + i, background=background, sigma=3.0) for i, s in enumerate(ac.build(name, dtype)[0])]


def feather_shows(m, views):
    """Fraction of the voxels at which some view has 0 < m < 1 while another view takes part: where a test says something about
    the feather.  ``m``, ``views``: the oracle's resampled tile weights and views (NaN where a view does not take part)."""
    part = ~np.isnan(views)
    partial = part & (m > 0) & (m < 1)
    return float((partial.any(0) & (part.sum(0) >= 2)).mean())
