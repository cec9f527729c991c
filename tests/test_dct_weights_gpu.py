"""GPU: DCT-entropy fusion weights (weights.content_based_dct, csrc/mvs_dct_weights.hip).  The standalone weights on
both quality paths against the reference's recorded outputs (tests/golden/dct_weights_ref.npz); fuse_np with the GPU
weights against fuse_np with the numpy / scipy restatement as a host callable (tests/dct_oracle.py); single-view chunks,
ignored weights, chunked fuse() in memory, to Zarr, on the device and from device arrays; and the reference's own
known-answer test (a sharp view wins over a blurred one)."""
import os

import numpy as np
import pytest
from scipy.ndimage import gaussian_filter

from tests import dct_oracle as do
from tests.helpers import assert_fused_close, bb_to_dicts, sim_to_view, squeeze_field, union_bb

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(os.path.dirname(__file__), "golden", "dct_weights_ref.npz"))


@pytest.fixture(params=["lds", "general"])
def quality_path(request, hip_device):
    from multiview_stitcher_amd import _lib

    _lib.set_option("dct_general", 1 if request.param == "general" else 0, hip_device)
    yield request.param
    _lib.set_option("dct_general", 0, hip_device)


@pytest.mark.parametrize("name", sorted(do.cases()))
def test_standalone_weights_match_reference(hip_device, quality_path, name):
    from multiview_stitcher_amd import weights

    views, kw = do.cases()[name]
    w, q = weights.content_based_dct(views, device=hip_device, return_quality=True, **kw)
    want_q = do.quality_maps(views, **kw)
    scale = max(float(np.nanmax(np.abs(want_q))), 1e-30)
    assert q.shape == want_q.shape
    np.testing.assert_allclose(q, want_q, rtol=0, atol=1e-5 * scale, equal_nan=True)
    np.testing.assert_allclose(do.shifted(q), FIX[f"qs/{name}"], rtol=0, atol=1e-5 * scale, equal_nan=True)
    assert w.dtype == np.float32 and w.shape == views.shape
    np.testing.assert_allclose(w, FIX[f"w/{name}"], rtol=0, atol=1e-5, equal_nan=True)


def test_device_array_in_and_out(hip_device):
    from multiview_stitcher_amd import weights
    from multiview_stitcher_amd.device import DeviceArray, is_device_array

    views, kw = do.cases()["3d_dict"]
    got = weights.content_based_dct(DeviceArray.from_host(views, hip_device), device=hip_device, **kw)
    assert is_device_array(got)
    np.testing.assert_array_equal(got.get(), weights.content_based_dct(views, device=hip_device, **kw))


def _tiles(ndim, dtype, rotate=False):
    """Tiles of one ground truth, each blurred differently (distinct block qualities), with affine params."""
    from multiview_stitcher_amd import sample_data

    shape = (12, 40, 44) if ndim == 3 else (52, 60)
    tiles = (1, 2, 2) if ndim == 3 else (2, 2)
    overlap = (0, 14, 16) if ndim == 3 else (18, 20)
    sims, _, _ = sample_data.generate_tiled_dataset(ndim=ndim, tile_shape=shape, tiles=tiles, overlap=overlap, max_jitter=0,
                                                    dtype=np.float32)
    sims = [squeeze_field(s) for s in sims]
    hi = 250.0 if dtype == np.uint8 else 4000.0
    for i, s in enumerate(sims):
        a = gaussian_filter(np.asarray(s.data, np.float64), 0.3 + 0.9 * i)
        a = a / max(a.max(), 1e-9) * hi
        s.data = a.astype(dtype)
    params = [np.eye(ndim + 1) for _ in sims]
    params[1][ndim - 2:ndim, ndim] = [0.5, -1.25]
    if rotate:
        t = np.deg2rad(7.0)
        r = np.eye(ndim + 1)
        r[ndim - 2:ndim, ndim - 2:ndim] = [[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]]
        c = np.zeros(ndim + 1)
        c[:ndim] = np.array(shape) / 2
        sh, shb = np.eye(ndim + 1), np.eye(ndim + 1)
        sh[:ndim, ndim], shb[:ndim, ndim] = c[:ndim], -c[:ndim]
        params[2] = sh @ r @ shb @ params[2]
    return sims, params


def _fuse_both(sims, params, ndim, wkw, **extra):
    from multiview_stitcher_amd import fusion

    sd = ["z", "y", "x"][-ndim:]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = bb_to_dicts(union_bb(bbs, params, np.ones(ndim)), sd)
    fvb = [bb_to_dicts(b, sd) for b in bbs]
    got = fusion.fuse_np(sims, params, out_bb, full_view_bbs=fvb, weights_func=fusion.content_based_dct, weights_func_kwargs=wkw, **extra)
    want = fusion.fuse_np(sims, params, out_bb, full_view_bbs=fvb, weights_func=do.content_based_dct, weights_func_kwargs=wkw, **extra)
    return got, want


@pytest.mark.parametrize("ndim,dtype,rotate", [(2, np.float32, False), (2, np.uint16, True), (3, np.uint16, False),
                                               (3, np.uint8, True), (3, np.float32, True)])
def test_fuse_np_matches_oracle_callable(hip_device, ndim, dtype, rotate):
    sims, params = _tiles(ndim, dtype, rotate)
    wkw = {"dct_size": 8} if ndim == 3 else {"dct_size": 16, "otf_support_fraction": 0.25}
    got, want = _fuse_both(sims, params, ndim, wkw)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    assert np.abs(got.astype(np.float64)).max() > 0
    if dtype == np.float32:
        assert_fused_close(got, want)
    else:
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1


def test_fuse_np_l1_branch_and_trim(hip_device):
    sims, params = _tiles(2, np.float32)
    got, want = _fuse_both(sims, params, 2, {"dct_size": 12, "otf_support_fraction": None, "exponent": 2.0},
                           trim_overlap_in_pixels=3)
    assert_fused_close(got, want)


def test_single_view_chunk_fuses_to_zero(hip_device):
    from multiview_stitcher_amd import fusion

    sims, params = _tiles(2, np.uint16)
    sd = ["y", "x"]
    view, bb = sim_to_view(sims[0])
    out_bb = bb_to_dicts(union_bb([bb], params[:1], np.ones(2)), sd)
    plain = fusion.fuse_np(sims[:1], params[:1], out_bb, full_view_bbs=[bb_to_dicts(bb, sd)])
    got = fusion.fuse_np(sims[:1], params[:1], out_bb, full_view_bbs=[bb_to_dicts(bb, sd)], weights_func=fusion.content_based_dct)
    assert plain.max() > 0
    assert got.shape == plain.shape and not got.any()


def test_max_fusion_ignores_dct_weights(hip_device):
    from multiview_stitcher_amd import fusion

    sims, params = _tiles(3, np.uint16, True)
    sd = ["z", "y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = bb_to_dicts(union_bb(bbs, params, np.ones(3)), sd)
    fvb = [bb_to_dicts(b, sd) for b in bbs]
    a = fusion.fuse_np(sims, params, out_bb, full_view_bbs=fvb, fusion_func=fusion.max_fusion, weights_func=fusion.content_based_dct)
    b = fusion.fuse_np(sims, params, out_bb, full_view_bbs=fvb, fusion_func=fusion.max_fusion)
    np.testing.assert_array_equal(a, b)


def test_output_on_backend_and_out(hip_device):
    from multiview_stitcher_amd import fusion
    from multiview_stitcher_amd.device import DeviceArray, is_device_array

    sims, params = _tiles(3, np.uint16)
    host, _ = _fuse_both(sims, params, 3, {"dct_size": 8})
    dsims = [s.copy(data=DeviceArray.from_host(np.asarray(s.data), hip_device)) for s in sims]
    sd = ["z", "y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = bb_to_dicts(union_bb(bbs, params, np.ones(3)), sd)
    fvb = [bb_to_dicts(b, sd) for b in bbs]
    dev = fusion.fuse_np(dsims, params, out_bb, full_view_bbs=fvb, weights_func=fusion.content_based_dct,
                         weights_func_kwargs={"dct_size": 8}, output_on_backend=True)
    assert is_device_array(dev)
    np.testing.assert_array_equal(dev.get(), host)


def _mosaic(ndim=3):
    from multiview_stitcher_amd import sample_data

    sims, _, _ = sample_data.generate_tiled_dataset(ndim=ndim, tile_shape=(10, 30, 34) if ndim == 3 else (40, 44),
                                                    tiles=(1, 2, 2) if ndim == 3 else (2, 2), overlap=(0, 10, 12) if ndim == 3 else (12, 12),
                                                    max_jitter=0, dtype=np.uint16)
    for i, s in enumerate(sims):
        a = gaussian_filter(np.asarray(s.data, np.float64), 0.3 + 0.9 * i)
        s.data = (a / a.max() * 4000).astype(np.uint16)
    return sims


def test_chunked_fuse_matches_oracle_callable(hip_device, tmp_path):
    from multiview_stitcher_amd import fusion, sample_data
    from multiview_stitcher_amd.device import DeviceArray, is_device_array

    key = sample_data.METADATA_TRANSFORM_KEY
    sims = _mosaic()
    chunks = {"z": 10, "y": 24, "x": 20}
    wkw = {"dct_size": 8}
    kw = dict(transform_key=key, weights_func_kwargs=wkw, output_chunksize=chunks, device=hip_device)
    got = fusion.fuse(sims, weights_func=fusion.content_based_dct, **kw)
    want = fusion.fuse(sims, weights_func=do.content_based_dct, **kw)
    g, w = np.asarray(got.data), np.asarray(want.data)
    assert g.shape == w.shape and g.max() > 0
    assert np.abs(g.astype(np.int64) - w.astype(np.int64)).max() <= 1
    zgot = fusion.fuse(sims, weights_func=fusion.content_based_dct, output_zarr_url=str(tmp_path / "dct.zarr"), **kw)
    np.testing.assert_array_equal(np.asarray(zgot.data), g)
    dev = fusion.fuse(sims, weights_func=fusion.content_based_dct, output_on_backend=True, **kw)
    assert is_device_array(dev.data)
    np.testing.assert_array_equal(dev.data.get().reshape(g.shape), g)
    dsims = [s.copy(data=DeviceArray.from_host(np.asarray(s.data), hip_device)) for s in sims]
    dgot = fusion.fuse(dsims, weights_func=fusion.content_based_dct, **kw)
    np.testing.assert_array_equal(np.asarray(dgot.data), g)


def test_reference_kat_prefers_sharp_view(hip_device):
    """_tests/test_weights.py:136-165 of the reference, restated (differences in float)."""
    from multiview_stitcher_amd import fusion, sample_data
    from multiview_stitcher_amd import spatial_image_utils as si_utils

    key = sample_data.METADATA_TRANSFORM_KEY
    rng = np.random.RandomState(0)
    sharp = rng.randint(0, 256, size=(64, 64)).astype(np.uint16)
    blurred = gaussian_filter(sharp.astype(np.float32), sigma=2.0).astype(np.uint16)
    sims = [si_utils.get_sim_from_array(a, dims=["y", "x"], transform_key=key) for a in (sharp, blurred)]
    fused = fusion.fuse(sims, transform_key=key, weights_func=fusion.content_based_dct,
                        weights_func_kwargs={"dct_size": {"y": 16, "x": 16}, "exponent": 1.0},
                        output_chunksize={"y": 32, "x": 32}, device=hip_device)
    f = np.asarray(fused.data).squeeze().astype(np.float64)
    assert f.shape == sharp.shape
    assert np.mean((f - sharp) ** 2) < np.mean((blurred.astype(np.float64) - sharp) ** 2)
