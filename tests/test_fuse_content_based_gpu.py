"""GPU: content-based fusion (csrc/mvs_gauss.hip, plan: csrc/mvs_cb_plan.h) against the oracle's fuse_np on the chunks that the default
path declines (tests/cb_cases.py; tests/test_cb_cases_host.py proves on the CPU that every case is what it is listed for here).  No
option forces a route: the chunk's own shape, views and sigmas do, and the counters of the bit-faithful passes say which one ran.
The branches and the cases that reach them:

  cb_fast_accepts_chunk  kCbViewCount: fan2d_12, fan3d_12, nine_views_3d;  kCbShortAxis: short_z3, short_z7, one_plane, short_z_default,
                         short_y_2d, stray_views, far_origin;  kCbMatrix: every turned case;  kCbRadius: radius_128
  cb_fast_accepts_boxes  kCbLine along y: long_y, mid_y
  cb_small == false      mask_normalize_kernel, cb_fuse_kernel, boxes read from global memory: fan2d_12 (2D), fan3d_12 and nine_views_3d (3D)
  cb_small == true       mask_normalize8_kernel, cb_fuse8_kernel: every other case
  cb_paired == true      gauss1d_pair_kernel, 2 * ndim launches per view with a box: every case but long_y and mid_y; the split y / z
                         passes in every 3D case and along y in the 2D ones
  cb_paired == false     without an option: long_y (y lines tap by tap in gauss1d_kernel, x lines in gauss1d_lds_kernel with
                         pos_fastest == 1), mid_y (y lines in gauss1d_lds_kernel with pos_fastest == 0); with cb_unpaired: the short axes
  cb_box_add             an empty reach (all-zero box, skipped by the passes) and a box of extent 1 along y: stray_views
  mvs_view_chunk_box     bounding box of the mapped slab, starting inside the chunk: shear_aniso, trimmed, lightsheet_pair, the fans
  valid masks            that are no boxes: every turned case; with NaN holes inside turned views: mirror_swap float32
  box_reflect            full < radius, several bounces: short_z3 (both filters), short_z7, short_z_default, short_y_2d, stray_views,
                         far_origin (second filter); full == 1: one_plane; b0 > 0 with len < full: every case with more than one view
  constant-tile short cut     decided per quantity (a box line that is the chunk line: mask 1 deep inside a view, value not constant):
                         long_y along y, the short axes along z; first sample invalid, tile not: shear_aniso, the fans
  lines of 1-2 samples   shear_aniso, trimmed (the corner view); stray_views (one row)
  cast_cb                uint8: fan2d_12, mirror_swap; uint16 and float32: most cases
  interpolation_order 0  fan2d_12, trimmed, mirror_swap
  trim                   3 with boxes that do not fill the chunk: trimmed; 8: long_y, mid_y; 64: radius_128; the halo of fuse(): lightsheet_pair
  offsets near 1e5       far_origin
  "sigma too large"      the error path of cb_scratch, and the context after it

Parity is ``helpers.assert_fused_close`` at its defaults: float32 within 1e-4 relative, integers within one count and only next to an
integer boundary of the reference's float result, the reference's own noise floor (``cb_cases.effective_noise_floor``) on at most 1 %
of the voxels.

Measured on an MI355X: the floor was needed at no voxel of any cell (beyond_plain_bar == 0 everywhere).  Against the oracle, end to end
-- float32: worst relative error; integers: voxels one count off (all next to a truncation boundary) of the voxels compared:

  fan2d_12         float32 1.0e-5 (order 0), 6.0e-6 (order 1); uint16 14 and 16 of 6723; uint8 0
  fan3d_12         float32 1.3e-5; uint16 107 of 72072
  shear_aniso      float32 1.4e-6; uint16 52 of 54432
  trimmed          float32 2.0e-6 (order 0), 7.3e-7 (order 1); uint16 12 and 35 of 22572
  far_origin       float32 1.8e-6
  mirror_swap      float32 4.8e-6 (order 0), 5.0e-6 (order 1); uint8 7 and 7 of 39050
  mirror_swap_one_rotated   uint16 32 of 35840
  lightsheet_pair  float32 5.6e-6; uint16 91 of 77440; in the four blocks of fuse(): uint16 17, 38, 25, 25 of 19360, float32 within the bar
  short_z3         float32 2.4e-7; uint16 0 of 25500        short_z7         float32 3.1e-7; uint16 1 of 45900
  one_plane        float32 3.3e-7; uint16 0 of 5100         short_z_default  float32 4.3e-6; uint16 13 of 161312
  short_y_2d       float32 3.0e-7; uint16 0 of 1020         stray_views      float32 5.1e-7; uint16 1 of 30600
  radius_128       float32 3.2e-7; uint16 2 of 20385        long_y           float32 1.6e-6; uint16 1 of 85900
  mid_y            float32 4.0e-7; uint16 0 of 12680        nine_views_3d    float32 1.2e-6; uint16 6 of 131144

(The turned cases differ from the oracle by more than the grids do: their resampled views and blending weights come out of another
summation order of the coordinates.)  At kernel level -- the library's built-in result against fo.content_based and
fo.weighted_average_fusion of the device's own views and weights -- every one of the 22 turned cells had equal bits: worst relative
error 0, no integer voxel off.  Every cell runs in under 0.3 s.
"""
import functools

import numpy as np
import pytest

from oracle import fuse_oracle as fo
from tests import cb_cases as cc
from tests.helpers import assert_fused_close, bb_to_dicts, fused_close_stats, same_bits, sim_to_view
from tests.test_fuse_gpu import _assert_cb_float_close

pytestmark = pytest.mark.gpu

CELLS = cc.cells()
ROTATED_CELLS = [c for c in CELLS if c[0] in cc.ROTATED]
COUNTERS = ("cb_line_launches", "cb_exact_chunks", "cb_exact_large_chunks", "cb_exact_paired_launches", "cb_exact_lds_launches",
            "cb_exact_tap_launches")


def _reset_counters():
    from multiview_stitcher_amd import _lib

    for key in COUNTERS:
        _lib.get_counter(key, reset=True)


def _read_counters():
    from multiview_stitcher_amd import _lib

    return {key: int(_lib.get_counter(key)) for key in COUNTERS}


def _planned(name, calls=1):
    return dict({k: calls * v for k, v in cc.plan(name)["counters"].items()}, cb_line_launches=0)


def _fuse(cell, sims=None, **more):
    """fusion.fuse_np of a cell with the built-in content-based weights."""
    from multiview_stitcher_amd import fusion

    name, dtype, order = cell
    built, params, out_bb, sigmas, kw = cc.build(name, dtype)
    sd = ["z", "y", "x"][-len(out_bb["shape"]):]
    fvb = [bb_to_dicts(sim_to_view(s)[1], sd) for s in built]
    more.setdefault("weights_func", fusion.content_based)
    return fusion.fuse_np(list(sims if sims is not None else built), list(params), bb_to_dicts(out_bb, sd), full_view_bbs=fvb,
                          weights_func_kwargs=cc.sigma_kwargs(sigmas), interpolation_order=order, **kw, **more)


@functools.lru_cache(maxsize=None)
def _library(cell):
    """The library's result of a cell and the counters of that one call.  Computed once; leave it unchanged."""
    _reset_counters()
    got = _fuse(cell)
    return got, _read_counters()


def _worst(got, want_f):
    """Worst error against the oracle's float result in units of the float bar (1e-4 relative, values below 1e-3 of the range: of that)."""
    rng = float(np.abs(want_f).max() or 1.0)
    return float((np.abs(got.astype(np.float64) - want_f) / np.maximum(np.abs(want_f), 1e-3 * rng)).max())


@pytest.mark.parametrize("cell", CELLS, ids=cc.cell_id)
def test_content_based_matches_oracle(hip_device, cell):
    name, dtype, order = cell
    want, want_f, _, floor = cc.oracle(name, dtype, order)
    got, counters = _library(cell)
    assert counters == _planned(name), (counters, _planned(name))
    assert got.shape == want.shape and got.dtype == want.dtype
    if np.dtype(dtype).kind == "f":
        print(f"{cc.cell_id(cell)}: worst relative error {_worst(got, want_f):.3e}")
    stats = assert_fused_close(got, want, want_f, noise_floor=floor)
    print(f"{cc.cell_id(cell)}: {stats}")
    assert np.isfinite(got.astype(np.float64)).all() and float((got != 0).mean()) >= 0.3, stats


@pytest.mark.parametrize("cell", ROTATED_CELLS, ids=cc.cell_id)
def test_built_in_weights_match_the_oracle_on_the_device_s_own_views(hip_device, cell):
    """Kernel level: the resampled views and normalised blending weights as the device makes them (a recording weights_func gets
    them), fo.content_based and fo.weighted_average_fusion of those arrays on the CPU, and the library's built-in result against
    that -- without a noise floor: both sides classify the same numbers."""
    name, dtype, order = cell
    _, _, _, sigmas, kw = cc.build(name, dtype)
    seen = {}

    def record(transformed_views, blending_weights, sigma_1, sigma_2):
        seen["views"], seen["blend"] = np.array(transformed_views, np.float32), np.array(blending_weights, np.float32)
        return np.ones(transformed_views.shape, np.float32)

    _fuse(cell, weights_func=record)
    views, blend = seen["views"], seen["blend"]
    near = (blend > 1e-7 * (1 - 1e-3)) & (blend < 1e-7 * (1 + 1e-3))
    assert not near.any(), f"{int(near.sum())} normalised weights at the 1e-7 threshold: the case needs another seed"
    with np.errstate(all="ignore"):
        fused = fo.weighted_average_fusion(views, blend, fo.content_based(views, blend, *sigmas))
    trim = kw.get("trim_overlap_in_pixels", 0)
    if trim:
        fused = fused[(slice(trim, -trim),) * fused.ndim]
    want_f = np.nan_to_num(fused)
    want = want_f.astype(dtype)
    got, _ = _library(cell)
    assert got.shape == want.shape
    if np.dtype(dtype).kind == "f":
        print(f"{cc.cell_id(cell)}: worst relative error {_worst(got, want_f):.3e}")
        _assert_cb_float_close(got, want)
    else:
        print(f"{cc.cell_id(cell)}: {fused_close_stats(got, want, want_f)}")


def test_two_runs_give_equal_bits(hip_device):
    cell = ("fan3d_12", cc.F32, 1)
    assert same_bits(_fuse(cell), _library(cell)[0])


@pytest.mark.parametrize("dtype", [cc.U16, cc.F32], ids=lambda d: d.name)
def test_strided_device_windows_equal_host_slabs(hip_device, dtype):
    """shear_aniso with a window of every tile: host slabs and a host result against zero-copy strided device windows and a device
    result."""
    from multiview_stitcher_amd import device

    cell = ("shear_aniso", dtype, 1)
    sims = cc.build("shear_aniso", dtype)[0]
    window = {"z": slice(1, None), "y": slice(2, None), "x": slice(3, None)}
    host = _fuse(cell, sims=[s.isel(window) for s in sims])
    _reset_counters()
    dev = _fuse(cell, sims=[device.to_device(s, hip_device).isel(window) for s in sims], output_on_backend=True)
    assert _read_counters() == _planned("shear_aniso")
    assert device.is_device_array(dev) and same_bits(host, dev.get())
    assert float((host != 0).mean()) >= 0.3 and not same_bits(host, _library(cell)[0])      # (the windows leave voxels out)


@pytest.mark.parametrize("dtype", [cc.U16, cc.F32], ids=lambda d: d.name)
@pytest.mark.parametrize("name", cc.SHORT_AXIS)
def test_short_axes_separate_passes_equal_paired_passes(hip_device, name, dtype):
    """Option cb_unpaired (separate value and mask passes, gauss1d_lds_kernel) changes no bit of a chunk with a short axis."""
    from multiview_stitcher_amd import _lib

    cell = (name, dtype, 1)
    paired, _ = _library(cell)
    _lib.set_option("cb_unpaired", 1)
    try:
        _reset_counters()
        separate = _fuse(cell)
        counters = _read_counters()
    finally:
        _lib.set_option("cb_unpaired", 0)
    planned = _planned(name)
    assert counters["cb_exact_paired_launches"] == 0 and counters["cb_exact_chunks"] == 1 and counters["cb_line_launches"] == 0
    assert counters["cb_exact_lds_launches"] + counters["cb_exact_tap_launches"] == 2 * planned["cb_exact_paired_launches"]
    assert same_bits(separate, paired)


@pytest.mark.parametrize("dtype", [cc.U16, cc.F32], ids=lambda d: d.name)
def test_chunked_fuse_of_lightsheet_pair(hip_device, dtype):
    """fusion.fuse() in 2 x 2 chunks along y and x with the content-based halo (2 * sigma_2 = 6): every block against the oracle's
    fuse_np on the block's box plus halo, trimmed -- the reflecting borders make the result depend on the chunking, so the oracle
    follows it."""
    from multiview_stitcher_amd import fusion, spatial_image_utils as si

    sims, params, out_bb, sigmas, _ = cc.build("lightsheet_pair", dtype)
    sd = ["z", "y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    full = [si.get_sim_from_array(v["data"], dims=sd, scale=dict(zip(sd, v["spacing"].tolist())), translation=dict(zip(sd, v["origin"].tolist())),
                                  affine=p, transform_key="k") for v, p in zip(views, params)]
    shape = [int(n) for n in out_bb["shape"]]
    block = [shape[0], shape[1] // 2, shape[2] // 2]
    halo = int(2 * sigmas[1])
    _reset_counters()
    fused = fusion.fuse(full, transform_key="k", output_stack_properties=bb_to_dicts(out_bb, sd), output_chunksize=dict(zip(sd, block)),
                        weights_func=fusion.content_based, weights_func_kwargs=cc.sigma_kwargs(sigmas), merge_chunks=False)
    counters = _read_counters()
    assert counters["cb_exact_chunks"] == 4 and counters["cb_line_launches"] == 0 and counters["cb_exact_paired_launches"] == 4 * 2 * 6, counters
    got = np.asarray(fused.data).reshape(shape)
    assert got.dtype == np.dtype(dtype)
    for iy in range(2):
        for ix in range(2):
            start = np.array([0, iy * block[1], ix * block[2]])
            box = fo.bb(out_bb["origin"] + (start - halo) * out_bb["spacing"], out_bb["spacing"], np.array(block) + 2 * halo)
            want, want_f, dbg = fo.fuse_np(list(views), list(params), box, weights="content_based", weights_kwargs=cc.sigma_kwargs(sigmas),
                                           full_view_bbs=list(bbs), trim_overlap_in_pixels=halo, return_debug=True)
            part = got[tuple(slice(int(a), int(a) + n) for a, n in zip(start, block))]
            stats = assert_fused_close(part, want, want_f, noise_floor=cc.effective_noise_floor(dbg, want_f, sigmas))
            print(f"lightsheet_pair-{np.dtype(dtype).name} block ({iy}, {ix}): {stats}")
            assert float((part != 0).mean()) >= 0.3


def test_sigma_too_large_is_an_error_and_the_context_goes_on(hip_device):
    """The taps of both filters travel in one block of at most 32 KiB (4096 float64): sigma_1 = 1 and sigma_2 = 512 have 9 + 4097.
    The call fails with the library's error before any filter runs, and the next call on the context gives an earlier result bit
    for bit."""
    from multiview_stitcher_amd import _lib, fusion

    assert (2 * cc.radius(1.0) + 1) + (2 * cc.radius(512.0) + 1) > 32 * 1024 // 8
    cell = ("short_y_2d", cc.F32, 1)
    before, _ = _library(cell)
    sims, params, out_bb, _, kw = cc.build(*cell[:2])
    sd = ["y", "x"]
    with pytest.raises(_lib.MvsError, match="sigma too large"):
        fusion.fuse_np(list(sims), list(params), bb_to_dicts(out_bb, sd), full_view_bbs=[bb_to_dicts(sim_to_view(s)[1], sd) for s in sims],
                       weights_func=fusion.content_based, weights_func_kwargs={"sigma_1": 1.0, "sigma_2": 512.0}, **kw)
    assert same_bits(_fuse(cell), before)
