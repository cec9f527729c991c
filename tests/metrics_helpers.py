"""Shared by tests/test_metrics_host.py and tests/test_metrics_gpu.py: one tile described once, as the package's multiscale image
and as the plain view of tests/metrics_oracle.py."""
import numpy as np

from multiview_stitcher_amd import msi_utils
from multiview_stitcher_amd import spatial_image_utils as si

SDIMS = ["z", "y", "x"]


def translation_affine(shift):
    a = np.eye(len(shift) + 1)
    a[:-1, -1] = shift
    return a


def make_tile(data, affines, origin=None, spacing=None, scale_factors=None, c_coords=None):
    """(msim, oracle view) of a tile: ``data`` is spatial, or (c, spatial...) with ``c_coords``; ``affines``: {key: matrix}."""
    ndim = data.ndim - (1 if c_coords is not None else 0)
    sdims = SDIMS[-ndim:]
    origin = np.zeros(ndim) if origin is None else np.asarray(origin, dtype=float)
    spacing = np.ones(ndim) if spacing is None else np.asarray(spacing, dtype=float)
    keys = list(affines)
    sim = si.get_sim_from_array(data, dims=(["c"] if c_coords is not None else []) + sdims, scale=dict(zip(sdims, spacing)),
                                translation=dict(zip(sdims, origin)), affine=affines[keys[0]], transform_key=keys[0], c_coords=c_coords)
    for k in keys[1:]:
        si.set_sim_affine(sim, np.asarray(affines[k], dtype=float), transform_key=k)
    msim = msi_utils.get_msim_from_sim(sim, scale_factors=scale_factors)
    view = {"data": data if c_coords is None else data[0], "origin": origin, "spacing": spacing,
            "affines": {k: np.asarray(a, dtype=float) for k, a in affines.items()}}
    return msim, view


def assert_same_structure(got, want):
    """Same pairs, candidate and metric keys, the same ``None`` boxes, NaN in the same places."""
    assert set(got) == {"pairs", "bboxes", "summary"}
    assert set(got["pairs"]) == set(want["pairs"]) and set(got["bboxes"]) == set(want["bboxes"])
    for p in want["pairs"]:
        assert (got["bboxes"][p] is None) == (want["bboxes"][p] is None), p
        if want["bboxes"][p] is not None:
            for k in ("lower", "upper"):
                assert np.array_equal(got["bboxes"][p][k], want["bboxes"][p][k]), (p, k, got["bboxes"][p][k], want["bboxes"][p][k])
        assert set(got["pairs"][p]) == set(want["pairs"][p])
        for q in want["pairs"][p]:
            assert set(got["pairs"][p][q]) == set(want["pairs"][p][q])
            for k, v in want["pairs"][p][q].items():
                assert np.isnan(got["pairs"][p][q][k]) == np.isnan(v), (p, q, k, got["pairs"][p][q][k], v)
    assert set(got["summary"]) == set(want["summary"])
    for q in want["summary"]:
        assert set(got["summary"][q]) == set(want["summary"][q])
