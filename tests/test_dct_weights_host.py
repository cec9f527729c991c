"""CPU tests of the DCT-entropy fusion weights (weights.content_based_dct): the numpy / scipy restatement against the
reference's recorded outputs, the builtin mapping, required_overlap, fuse()'s halo and the C ABI of the new entries."""
import ctypes
import os
import time

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, fusion, weights
from tests import dct_oracle as do

FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "dct_weights_ref.npz"))


@pytest.mark.parametrize("name", sorted(do.cases()))
def test_restatement_matches_reference(name):
    views, kw = do.cases()[name]
    q = do.quality_maps(views, **kw)
    qs = do.shifted(q)
    want_qs = FIX[f"qs/{name}"]
    assert qs.shape == want_qs.shape
    scale = max(float(np.nanmax(np.abs(q))), 1e-30)
    np.testing.assert_allclose(qs, want_qs, rtol=0, atol=1e-5 * scale, equal_nan=True)
    w = do.content_based_dct(views, **kw)
    np.testing.assert_allclose(w, FIX[f"w/{name}"], rtol=0, atol=1e-5, equal_nan=True)


def test_single_view_gets_zero_weight_everywhere():
    views, kw = do.cases()["single_view"]
    assert float(np.max(FIX["w/single_view"])) == 0.0
    assert float(np.max(do.content_based_dct(views, **kw))) == 0.0


def test_l1_branch_with_fractional_exponent_is_nan():
    """The L1 branch's entropy is never positive (Jensen), so a fractional exponent gives NaN (the reference's host path
    raises there, taking a complex power of a Python float); the restatement keeps the NaN."""
    views, _ = do.cases()["l1_exp1"]
    q = do.quality_maps(views, dct_size=16, otf_support_fraction=None, exponent=0.5)
    assert np.isnan(q).any()
    assert np.all(do.quality_maps(views, dct_size=16, otf_support_fraction=None) <= 0)


@pytest.mark.parametrize("i", range(len(do.overlap_cases())))
def test_required_overlap_matches_reference(i):
    kw, ocs = do.overlap_cases()[i]
    want = FIX[f"overlap/{i}"].tolist()
    for fn in (do.required_overlap, weights.content_based_dct.required_overlap, fusion.content_based_dct.required_overlap):
        got = fn(dict(kw, output_chunksize=ocs))
        assert [got[d] for d in sorted(got)] == want


def test_builtin_mapping_and_exports():
    assert fusion.builtin("content_based_dct") is weights.content_based_dct
    assert fusion.content_based_dct is weights.content_based_dct
    ref_like = lambda transformed_views, dct_size=32: None  # noqa: E731
    ref_like.__name__ = "content_based_dct"
    assert fusion.builtin(ref_like) is weights.content_based_dct
    assert fusion.has_keyword(fusion.content_based_dct, "output_chunksize")


def test_fuse_halo_injects_output_chunksize():
    """fuse()'s halo (_core.py:1194-1222): the requested chunk size goes into required_overlap's kwargs of functions that accept it."""
    sd = ["z", "y", "x"]
    ocs = {"z": 16, "y": 64, "x": 24}
    got = fusion._halo_overlap(0, sd, [(fusion.content_based_dct, None), (fusion.weighted_average_fusion, None)], ocs)
    assert got == {"z": 16, "y": 32, "x": 24} == do.required_overlap({"output_chunksize": ocs})
    got = fusion._halo_overlap({"z": 20, "y": 2, "x": 2}, sd, [(fusion.content_based_dct, {"dct_size": 8}), (None, None)], ocs)
    assert got == {"z": 20, "y": 8, "x": 8}
    # functions without the keyword see their kwargs unchanged (content_based: 2 * sigma_2)
    assert fusion._halo_overlap(0, sd, [(fusion.content_based, {"sigma_2": 5})], ocs) == {"z": 10, "y": 10, "x": 10}
    assert fusion._halo_overlap(3, ["y", "x"], [(None, None)], {"y": 8, "x": 8}) == {"y": 3, "x": 3}


def test_dct_opts_layout_and_exports():
    assert ctypes.sizeof(_lib.mvs_dct_opts_t) == 24 + 24 + 8 + 8 + 4 + 4
    assert _lib.mvs_dct_opts_t.exponent.offset == 48 and _lib.mvs_dct_opts_t.has_otf.offset == 64
    lib = _lib.load()
    for name in ("mvs_fuse_chunk_dct", "mvs_content_dct_weights"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    o = weights.dct_opts(2, {"y": 16, "x": 12}, 2.0, None, {"y": 40, "x": 50})
    assert list(o.dct_size) == [1, 16, 12] and list(o.output_chunksize) == [1, 40, 50]
    assert o.has_otf == 0 and o.has_output_chunksize == 1 and o.exponent == 2.0


def test_restatement_cpu_time_of_the_default_chunk_slice():
    """Records the restatement's CPU cost on one 64 x 320 x 320 slab of two views."""
    rng = np.random.default_rng(0)
    views = rng.random((2, 64, 320, 320)).astype(np.float32)
    t = time.perf_counter()
    q = do.quality_maps(views)
    dt = time.perf_counter() - t
    assert q.shape == (2, 2, 10, 10)
    print(f"restatement quality pass on (2, 64, 320, 320): {dt:.2f} s")
