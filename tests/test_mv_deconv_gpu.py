"""GPU: multi-view deconvolution (fusion.multi_view_deconvolution, csrc/mvs_deconv.hip) against the numpy / scipy
restatement of the reference (tests/deconv_oracle.py): the direct function on both convolution paths, fuse_np against
the oracle chain resample + blending weights + restatement, a chunked fuse() (in memory and to Zarr) against the
per-chunk oracle composed into the mosaic, DeviceArray in / out, and the call frame the deconvolution shares with multi-band
fusion (trimmed host / device / caller-supplied results of both, bit for bit).  The edge cases (do.edge_cases(): tile edges, the
widest and tallest kernels, even and asymmetric kernels on both paths, thin chunks, voxels no view covers, 65 views)
run a few iterations each; tests/test_mv_deconv_host.py shows that each would catch the kernel mistakes it targets."""
import functools

import numpy as np
import pytest

from oracle import fuse_oracle as fo
from oracle import plan_oracle as po
from tests import deconv_oracle as do
from tests.helpers import bb_to_dicts, sim_to_view, squeeze_field, union_bb

pytestmark = pytest.mark.gpu

ITERATIONS = 10


def _close(got, want, rel=2e-4):
    scale = float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    assert err <= rel * scale, (err, scale, err / scale)


@pytest.fixture(params=["separable", "general"])
def conv_path(request, hip_device):
    from multiview_stitcher_amd import _lib

    _lib.set_option("deconv_general", 1 if request.param == "general" else 0, hip_device)
    yield request.param
    _lib.set_option("deconv_general", 0, hip_device)


@pytest.mark.parametrize("name", sorted(do.cases()))
def test_direct_call_matches_restatement(hip_device, conv_path, name):
    from multiview_stitcher_amd import fusion

    views, blend, kw = do.cases()[name]
    want = do.deconvolve(views, blend, n_iterations=ITERATIONS, **kw)
    got = fusion.multi_view_deconvolution(views, blend, n_iterations=ITERATIONS, device=hip_device, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape
    if kw.get("sample_boundary_erosion_px"):
        np.testing.assert_array_equal(got == 0, want == 0)
    _close(got, want)


@functools.lru_cache(maxsize=None)
def _edge_cases():
    return do.edge_cases()


@functools.lru_cache(maxsize=None)
def _edge_want(name, dtype=np.float32):
    """The restatement's result of an edge case (computed once for both paths); integer dtypes take the views with
    NaN -> 0 cast to that dtype."""
    views, blend, kw, it = _edge_cases()[name]
    if np.dtype(dtype) != np.float32:
        views = np.nan_to_num(views).astype(dtype)
    return views, do.deconvolve(views, blend, n_iterations=it, **kw)


@pytest.mark.parametrize("name", sorted(do.edge_cases()))
def test_edge_case_matches_restatement(hip_device, conv_path, name):
    from multiview_stitcher_amd import fusion

    views, blend, kw, it = _edge_cases()[name]
    _, want = _edge_want(name)
    got = fusion.multi_view_deconvolution(views, blend, n_iterations=it, device=hip_device, **kw)
    assert got.dtype == want.dtype and got.shape == want.shape
    if kw.get("sample_boundary_erosion_px"):
        np.testing.assert_array_equal(got == 0, want == 0)
    _close(got, want)


@pytest.mark.parametrize("name", ["3d_rank1_even_OPTIMIZATION_I", "3d_direct_even", "2d_uncovered_erosion3_lambda1"])
def test_edge_case_integer_output(hip_device, conv_path, name):
    from multiview_stitcher_amd import fusion

    _, blend, kw, it = _edge_cases()[name]
    views, want = _edge_want(name, np.uint16)
    got = fusion.multi_view_deconvolution(views, blend, n_iterations=it, device=hip_device, **kw)
    assert got.dtype == want.dtype == np.uint16 and got.shape == want.shape
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1
    if kw.get("sample_boundary_erosion_px"):
        np.testing.assert_array_equal(got == 0, want == 0)


def test_separable_path_is_taken_for_gaussians(hip_device):
    """The default PSF and its compound kernels pass the rank-1 test (both tables present); a non-separable PSF does not."""
    from multiview_stitcher_amd import mv_deconv

    k1, k2, s1, s2 = mv_deconv._kernels(2, 3, None, "EFFICIENT_BAYESIAN", None, 0.8, 0.5)
    assert s1 is not None and s2 is not None and s1.shape == (2, 27)
    _, _, s1, s2 = mv_deconv._kernels(2, 2, do.cases()["2d_nonseparable"][2]["psfs"], "EFFICIENT_BAYESIAN", None, 0.8, 0.5)
    assert s1 is None and s2 is None


def test_uint16_direct_call_casts_like_astype(hip_device):
    from multiview_stitcher_amd import fusion

    views, blend, kw = do.cases()["3d_default"]
    v16 = np.nan_to_num(views).astype(np.uint16)
    want = do.deconvolve(v16, blend, n_iterations=ITERATIONS)
    got = fusion.multi_view_deconvolution(v16, blend, n_iterations=ITERATIONS, device=hip_device)
    assert got.dtype == np.uint16
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1


def test_uint8_direct_call_casts_like_astype(hip_device, conv_path):
    """uint8 views kept well below 255 (the result must not overshoot: numpy's out-of-range float -> uint cast is
    platform-dependent)."""
    from multiview_stitcher_amd import fusion

    views, blend, kw = do.cases()["3d_default"]
    v8 = (np.nan_to_num(views) * np.float32(0.5)).astype(np.uint8)
    assert v8.max() <= 120
    want = do.deconvolve(v8, blend, n_iterations=ITERATIONS)
    assert want.max() < 200
    got = fusion.multi_view_deconvolution(v8, blend, n_iterations=ITERATIONS, device=hip_device)
    assert got.dtype == np.uint8
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1


def _oracle_chunk(views, params, out_bb, full_bbs, trim, kw, dtype):
    """fuse_np of the reference with fusion_func=multi_view_deconvolution (_core.py:1608-1713)."""
    ims = np.stack([fo.transform_array(v["data"].astype(np.float32), np.linalg.inv(p), v["origin"], fb["spacing"], out_bb,
                                       order=1, cval=np.nan) for v, p, fb in zip(views, params, full_bbs)])
    ws = np.stack([fo.get_blending_weights(out_bb, fb, p) for fb, p in zip(full_bbs, params)])
    ws = fo.normalize_weights(ws * ~np.isnan(ims))
    kw = dict(kw)
    sdims = ["z", "y", "x"][-ims.ndim + 1:]
    kw.setdefault("output_spacing", dict(zip(sdims, np.asarray(out_bb["spacing"], dtype=float).tolist())))
    fused = do.deconvolve(ims, ws, **kw)
    if any(trim):
        fused = fused[tuple(slice(t, -t) if t else slice(None) for t in trim)]
    return np.nan_to_num(fused).astype(dtype)


def _rotated_pair(dtype, ndim=3):
    from multiview_stitcher_amd import spatial_image_utils as si

    rng = np.random.default_rng(3)
    shape = (10, 36, 40)[-ndim:]
    base = (rng.random(shape) * 200 + 50).astype(np.float32)
    from scipy import ndimage

    base = ndimage.gaussian_filter(base, 1.5) * 3
    if dtype == np.uint8:
        base = base * np.float32(110.0 / base.max())
    sims, params = [], []
    for i in range(2):
        arr = base.astype(dtype)
        s = si.get_sim_from_array(arr, dims=["z", "y", "x"][-ndim:], scale={d: 1.0 for d in "zyx"[-ndim:]},
                                  translation={d: 0.0 for d in "zyx"[-ndim:]})
        sims.append(squeeze_field(s))
        p = np.eye(ndim + 1)
        if i == 1:
            a = np.deg2rad(7.0)
            p[ndim - 2:ndim, ndim - 2:ndim] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
            p[:ndim, ndim] = [0.0] * (ndim - 2) + [3.3, -2.6]
        params.append(p)
    return sims, params


def _translated_pair(dtype):
    from multiview_stitcher_amd import sample_data

    sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=(10, 30, 34), tiles=(1, 1, 2), overlap=(0, 0, 12),
                                                    dtype=np.float32 if dtype == np.uint8 else dtype, max_jitter=0)
    sims = [squeeze_field(s) for s in sims]
    if dtype == np.uint8:        # values in [5, 115], so the result does not overshoot 255
        sims = [s.copy(data=(np.asarray(s.data) * np.float32(110.0) + np.float32(5.0)).astype(np.uint8)) for s in sims]
    params = [np.eye(4) for _ in sims]
    params[1][:3, 3] = [0.0, 0.4, -1.7]
    return sims, params


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.uint8])
@pytest.mark.parametrize("geometry", ["translated", "rotated"])
def test_fuse_np_matches_oracle_chain(hip_device, dtype, geometry):
    from multiview_stitcher_amd import fusion, spatial_image_utils as si

    sims, params = (_translated_pair if geometry == "translated" else _rotated_pair)(dtype)
    sdims = si.get_spatial_dims_from_sim(sims[0])
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = union_bb(bbs, params, np.ones(3))
    kw = {"n_iterations": ITERATIONS}
    want = _oracle_chunk(views, params, out_bb, bbs, (0, 2, 2), kw, dtype)
    got = fusion.fuse_np(list(sims), params, bb_to_dicts(out_bb, sdims), fusion_func=fusion.multi_view_deconvolution,
                         fusion_func_kwargs=kw, full_view_bbs=[bb_to_dicts(b, sdims) for b in bbs],
                         trim_overlap_in_pixels={"z": 0, "y": 2, "x": 2}, device=hip_device)
    assert got.dtype == want.dtype and got.shape == want.shape
    if dtype == np.uint8:
        assert want.max() < 200
    if dtype != np.float32:
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1
    else:
        _close(got, want)
    dev = fusion.fuse_np(list(sims), params, bb_to_dicts(out_bb, sdims), fusion_func=fusion.multi_view_deconvolution,
                         fusion_func_kwargs=kw, full_view_bbs=[bb_to_dicts(b, sdims) for b in bbs],
                         trim_overlap_in_pixels={"z": 0, "y": 2, "x": 2}, output_on_backend=True, device=hip_device)
    np.testing.assert_array_equal(dev.get(), got)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_fuse_np_2d_three_rotated_views(hip_device, dtype):
    """fuse_np in 2D with three rotated and shifted views: the union box has corners no view covers (weights 0 / 1,
    ratio 1) and every voxel of the chunk has its own mix of weights."""
    from multiview_stitcher_amd import fusion
    from multiview_stitcher_amd import spatial_image_utils as si
    from scipy import ndimage

    rng = np.random.default_rng(11)
    base = ndimage.gaussian_filter(rng.random((40, 46)) * 300.0, 1.0) + rng.random((40, 46)) * 40.0 + 20.0
    sims, params = [], []
    for angle, shift in ((0.0, (0.0, 0.0)), (9.0, (2.4, -3.1)), (-14.0, (-1.7, 2.6))):
        s = si.get_sim_from_array(base.astype(dtype), dims=["y", "x"], scale={"y": 1.0, "x": 1.0}, translation={"y": 0.0, "x": 0.0})
        sims.append(squeeze_field(s))
        a = np.deg2rad(angle)
        p = np.eye(3)
        p[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        p[:2, 2] = shift
        params.append(p)
    sdims = ["y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = union_bb(bbs, params, np.ones(2))
    kw = {"n_iterations": 4, "psf_type": "OPTIMIZATION_II", "sample_boundary_erosion_px": 1}
    want = _oracle_chunk(views, params, out_bb, bbs, (2, 2), kw, dtype)
    got = fusion.fuse_np(list(sims), params, bb_to_dicts(out_bb, sdims), fusion_func=fusion.multi_view_deconvolution,
                         fusion_func_kwargs=kw, full_view_bbs=[bb_to_dicts(b, sdims) for b in bbs],
                         trim_overlap_in_pixels={"y": 2, "x": 2}, device=hip_device)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert (want == 0).any() and (want > 0).mean() > 0.5       # uncovered corners, eroded to 0
    np.testing.assert_array_equal(got == 0, want == 0)
    if dtype == np.uint16:
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1
    else:
        _close(got, want)


def _params_of(sim, key):
    from multiview_stitcher_amd import spatial_image_utils as si

    p = np.asarray(si.get_affine_from_sim(sim, key), dtype=np.float64)
    return p.reshape((-1,) + p.shape[-2:])[0]


def _per_chunk_oracle(sims, fused, key, chunks, kw):
    """The mosaic that fuse() with ``fusion_func=multi_view_deconvolution`` should produce: the plan oracle's chunks
    (with the deconvolution's halo), each run through the oracle chain of fuse_np, trimmed and composed.  Returns the
    mosaic (in the fused result's dtype) and the number of chunks that had views."""
    from multiview_stitcher_amd import fusion, mv_graph
    from multiview_stitcher_amd import spatial_image_utils as si

    got_dtype = np.asarray(fused.data).dtype
    shape = np.asarray(fused.data).shape[-3:]
    sq = [squeeze_field(s) for s in sims]
    sdims = si.get_spatial_dims_from_sim(sq[0])
    params = [_params_of(s, key) for s in sims]
    bbs = [si.get_stack_properties_from_sim(s) for s in sq]
    osp = si.get_stack_properties_from_sim(squeeze_field(fused))
    halo = fusion.multi_view_deconvolution.required_overlap(kw)
    overlap = {d: halo for d in sdims}
    cbb, bidx = mv_graph.get_chunk_bbs(osp, chunks)
    cbb_ov = [cb | {"origin": {d: cb["origin"][d] - overlap[d] * osp["spacing"][d] for d in sdims}}
              | {"shape": {d: cb["shape"][d] + 2 * overlap[d] for d in sdims}} for cb in cbb]
    plan = po._build_spatial_fusion_plan(
        sparams=params, views_bb=bbs, output_stack_properties=osp, output_chunksize=chunks, output_chunk_bbs=cbb,
        output_chunk_bbs_with_overlap=cbb_ov, output_chunk_bbs_for_result=cbb, block_indices=bidx, overlap_in_pixels=overlap,
        trim_overlap=True, interpolation_order=1, sdims=sdims)
    want = np.zeros(shape, got_dtype)
    n_chunks = 0
    for entry in plan["per_chunk_entries"]:
        if not entry["views"]:
            continue
        n_chunks += 1
        views, vparams, fbbs = [], [], []
        for iv, obb in entry["views"]:
            slab = po._select_slab(sq[iv], obb, sdims)
            v, _ = sim_to_view(slab)
            views.append(v)
            vparams.append(params[iv])
            fbbs.append(fo.bb([bbs[iv]["origin"][d] for d in sdims], [bbs[iv]["spacing"][d] for d in sdims],
                              [bbs[iv]["shape"][d] for d in sdims]))
        ob = entry["output_bb_overlap"]
        out_bb = fo.bb([ob["origin"][d] for d in sdims], [ob["spacing"][d] for d in sdims], [ob["shape"][d] for d in sdims])
        chunk = _oracle_chunk(views, vparams, out_bb, fbbs, (halo,) * 3, kw, got_dtype)
        res = entry["output_bb_result"]
        lo = [int(round((res["origin"][d] - osp["origin"][d]) / osp["spacing"][d])) for d in sdims]
        want[tuple(slice(a, a + n) for a, n in zip(lo, chunk.shape))] = chunk
    return want, n_chunks


def test_fuse_chunked_mosaic_matches_per_chunk_oracle(hip_device, tmp_path):
    from multiview_stitcher_amd import fusion, sample_data

    key = sample_data.METADATA_TRANSFORM_KEY
    sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=(8, 28, 30), tiles=(2, 2, 2), overlap=(3, 8, 8),
                                                    max_jitter=0, dtype=np.uint16)
    kw = {"n_iterations": 4, "psf_type": "OPTIMIZATION_I"}
    chunks = {"z": 7, "y": 20, "x": 24}
    fused = fusion.fuse(sims, transform_key=key, fusion_func=fusion.multi_view_deconvolution, fusion_func_kwargs=kw,
                        output_chunksize=chunks, device=hip_device)
    got = np.asarray(fused.data).reshape(np.asarray(fused.data).shape[-3:])

    assert fusion.multi_view_deconvolution.required_overlap(kw) == 4
    want, n_chunks = _per_chunk_oracle(sims, fused, key, chunks, kw)
    assert n_chunks > 4
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1

    zfused = fusion.fuse(sims, transform_key=key, fusion_func=fusion.multi_view_deconvolution, fusion_func_kwargs=kw,
                         output_chunksize=chunks, output_zarr_url=str(tmp_path / "deconv.zarr"), device=hip_device)
    np.testing.assert_array_equal(np.asarray(zfused.data).reshape(got.shape), got)


def test_single_plane_chunks(hip_device):
    """fuse() with a z chunk of 1 on the views' z grid: every chunk is one plane plus the 4-voxel halo, thinner than the
    PSF (mirror boundaries wrap periodically there); the mosaic equals the per-chunk oracle."""
    from multiview_stitcher_amd import fusion, sample_data

    key = sample_data.METADATA_TRANSFORM_KEY
    sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=(4, 24, 26), tiles=(1, 2, 2), overlap=(0, 8, 8),
                                                    max_jitter=0, dtype=np.uint16)
    kw = {"n_iterations": 3}
    chunks = {"z": 1, "y": 24, "x": 24}
    fused = fusion.fuse(sims, transform_key=key, fusion_func=fusion.multi_view_deconvolution,
                        fusion_func_kwargs=kw, output_chunksize=chunks, device=hip_device)
    d = np.asarray(fused.data)
    assert d.shape[-3] == 4 and d.max() > 0
    got = d.reshape(d.shape[-3:])
    want, n_chunks = _per_chunk_oracle(sims, fused, key, chunks, kw)
    assert n_chunks >= 4 * 4
    assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1


def test_device_arrays_in_and_out(hip_device):
    from multiview_stitcher_amd import fusion
    from multiview_stitcher_amd.device import DeviceArray, is_device_array

    views, blend, kw = do.cases()["3d_lambda_erosion"]
    want = fusion.multi_view_deconvolution(views, blend, n_iterations=ITERATIONS, device=hip_device, **kw)
    got = fusion.multi_view_deconvolution(DeviceArray.from_host(views, hip_device), DeviceArray.from_host(blend, hip_device),
                                          n_iterations=ITERATIONS, device=hip_device, **kw)
    assert is_device_array(got) and got.dtype == np.float32
    np.testing.assert_array_equal(got.get(), want)


def _frame_run(entry, shape):
    """``run(trim, out_on_device, out=None)`` of one stack entry point on two views of ``shape`` with a uint16 result: the
    deconvolution with one iteration of the default 1.5-pixel Gaussian kernels, multi-band fusion with n_levels = 1."""
    from multiview_stitcher_amd import multiband, mv_deconv
    from multiview_stitcher_amd.device import DeviceArray

    def run(trim, out_on_device, out=None, device=None):
        ndim = len(shape)
        rng = np.random.default_rng(17)
        views = (rng.random((2,) + shape) * 900 + 50).astype(np.float32)
        views[0][..., :5] = np.nan
        views[1][..., -4:, :] = np.nan
        blend = (rng.random((2,) + shape) + 0.1).astype(np.float32)
        blend /= blend.sum(0)
        dv, dw = DeviceArray.from_host(views, device), DeviceArray.from_host(blend, device)
        if entry == "mv_deconv":
            kernels = mv_deconv._kernels(2, ndim, None, "EFFICIENT_BAYESIAN", None, 0.8, 0.5)
            return mv_deconv._run(dv, dw, ndim, kernels, 1, 0.0, 1e-4, 0, list(trim), np.uint16, out_on_device, device, out=out)
        return multiband._run(dv, dw, ndim, [0] * (3 - ndim) + [1] * ndim, [0, 0, 0], list(trim), np.uint16, out_on_device, device, out=out)

    return run


@pytest.mark.parametrize("shape,trim", [((24, 40), (2, 3)), ((6, 12, 20), (1, 2, 3))])
@pytest.mark.parametrize("entry", ["mv_deconv", "multiband"])
def test_stack_frame_trim_and_result_paths(hip_device, entry, shape, trim):
    """The frame both stack entry points share (csrc/mvs_stack_frame.h, _stack_ops.run_stack_call), called through ``_run`` with a
    non-zero trim and a uint16 result: the host result, the device result and the device result written into a caller's ``out``
    are bit-equal, of shape S - 2 trim, and equal to the interior of the untrimmed result."""
    from multiview_stitcher_amd.device import DeviceArray, is_device_array

    run = _frame_run(entry, shape)
    res_shape = tuple(s - 2 * t for s, t in zip(shape, trim))
    host = run(trim, False, device=hip_device)
    dev = run(trim, True, device=hip_device)
    mine = DeviceArray.empty(res_shape, np.uint16, hip_device)
    into = run(trim, True, out=mine, device=hip_device)
    assert isinstance(host, np.ndarray) and is_device_array(dev) and into is mine
    assert host.dtype == np.uint16 and host.shape == res_shape and tuple(dev.shape) == res_shape and dev.dtype == np.uint16
    assert host.tobytes() == dev.get().tobytes() == mine.get().tobytes()
    whole = run([0] * len(shape), False, device=hip_device)
    assert whole.shape == shape and whole.max() > 0
    interior = whole[tuple(slice(t, s - t) for s, t in zip(shape, trim))]
    assert np.array_equal(host, interior)
    with pytest.raises(ValueError, match="out must be a contiguous DeviceArray of the result shape and dtype"):
        run(trim, True, out=DeviceArray.empty(shape, np.uint16, hip_device), device=hip_device)
