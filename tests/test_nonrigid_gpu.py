"""GPU tests of the non-rigid tile refinement: mvs_block_match against the numpy restatement of tests/nonrigid_oracle.py and against
the two-pass NCC of the very samples mvs_resample writes, the bits of its rows, its refusals, mvs_field_warp against the float64
restatement, and fit_fields / apply_fields / fuse end to end.

Shapes are the smallest that reach every path: blocks of 12 with partial ones of 4 and 8, a search window that leaves the moving
tile, halfspaces through blocks, more blocks than one batch, rows of the warp below and off the 16-byte vectors (72, 130, 67)."""
import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _metric_ops, _nonrigid_ops, fusion, metrics, msi_utils, nonrigid
from multiview_stitcher_amd.device import DeviceArray, to_device
from multiview_stitcher_amd.transformation import resample_array
from tests import nonrigid_cases as nc
from tests import nonrigid_oracle as no
from tests.helpers import same_bits
from tests.intensity_helpers import DTYPES, texture
from tests.metrics_helpers import make_tile, translation_affine

pytestmark = pytest.mark.gpu


def match(c, blocks=None, fixed=None, moving=None, **kw):
    return _nonrigid_ops.block_match(c["fixed"] if fixed is None else fixed, c["moving"] if moving is None else moving, c["fixed_affine"],
                                     c["moving_affine"], c["blocks"] if blocks is None else blocks, c["radius"], c["halfspaces"], **kw)


# ---- moments against the oracle and against the materialised samples --------------------------------------------------------------
def materialised_ncc(c, device):
    """The NCC of every (block, shift) from the device's own samples: mvs_resample of the fixed grid and of the grown moving grid,
    the halfspace mask on the fixed one, and the host's two-pass float64 sums."""
    grid, r = c["grid_shape"], np.asarray(c["radius"])
    f = np.array(resample_array(c["fixed"], c["fixed_affine"][0], c["fixed_affine"][1], grid, order=1, cval=np.nan, device=device, out_on_device=False))
    f[~metrics.halfspace_mask(c["halfspaces"], tuple(grid))] = np.nan
    mm, mo_ = c["moving_affine"]
    m = np.asarray(resample_array(c["moving"], mm, mo_ - mm @ r, tuple(np.asarray(grid) + 2 * r), order=1, cval=np.nan, device=device, out_on_device=False))
    shifts = list(np.ndindex(*[2 * v + 1 for v in r]))
    out = np.zeros((len(c["blocks"]), len(shifts)))
    for b, (lo, n) in enumerate(c["blocks"]):
        fb = f[tuple(slice(a, a + k) for a, k in zip(lo, n))]
        for s, sh in enumerate(shifts):
            out[b, s] = metrics.normalized_cross_correlation(fb, m[tuple(slice(a + d, a + d + k) for a, d, k in zip(lo, sh, n))])
    return out


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("ndim", [2, 3])
def test_block_moments_match_the_oracle_and_the_materialised_ncc(hip_device, ndim, dtype_name):
    c = nc.match_case(ndim, dtype_name)
    # the input condition of the exact counts: no voxel on a halfspace plane, no coordinate within 1e-6 px of a tile border
    assert no.halfspace_clearance(c["blocks"], c["halfspaces"]) > 1e-9
    assert no.border_clearance(c["fixed_affine"], c["blocks"], (0,) * ndim, c["fixed"].shape) > 1e-6
    assert no.border_clearance(c["moving_affine"], c["blocks"], c["radius"], c["moving"].shape) > 1e-6
    want = nc.match_oracle(ndim, dtype_name)
    n = want[..., 0]
    assert {tuple(b) for b in c["blocks"][:, 1]} >= ({(4, 12, 8), (12, 12, 8), (4, 12, 12), (12, 12, 12)} if ndim == 3 else {(32, 13), (32, 32)})
    assert (n.max(axis=1) != n.min(axis=1)).sum() >= 3                 # part of the window outside the moving tile: n differs between shifts
    assert any(0 < n[b].max() < np.prod(c["blocks"][b, 1]) for b in range(len(n)))      # a halfspace cuts through a block
    got = match(c)
    assert got.shape == want.shape == (len(c["blocks"]), _nonrigid_ops.n_shifts(c["radius"]), 6)
    scale = float(np.nanmax(np.abs(c["fixed"].astype(np.float64))))
    print(f"ndim {ndim} {dtype_name}: n {n.min()}..{n.max()}, max mean diff {np.abs(got[..., 1:3] - want[..., 1:3]).max():.3g}")
    assert np.array_equal(got[..., 0], n)
    np.testing.assert_allclose(got[..., 1:3], want[..., 1:3], rtol=1e-5, atol=1e-4 * scale)
    assert np.all(got[got[..., 0] == 0] == 0)                          # rows without a pair are exactly zero
    # the same device samples, summed by the kernel and by the host: n <= 1e5 terms, 1e-9 (tests/test_metrics_gpu.py, test (b))
    mat = materialised_ncc(c, hip_device)
    ker = nonrigid.ncc_of_moments(got)
    assert np.array_equal(np.isnan(ker), np.isnan(mat))
    ok = ~np.isnan(mat)
    print(f"  kernel against materialised NCC: max diff {np.abs(ker[ok] - mat[ok]).max():.3g} over {ok.sum()} rows")
    assert np.abs(ker[ok] - mat[ok]).max() <= 1e-9
    assert all(_metric_ops.ncc_from_moments(got[0, s]) == ker[0, s] or np.isnan(ker[0, s]) for s in range(0, got.shape[1], 17))


def test_block_without_a_pair_gives_zero_rows(hip_device):
    c = nc.match_case(2, "u16")
    everything_masked = dict(c, halfspaces=np.array([[0.0, 0.0, 1.0]]))
    got = match(everything_masked)
    assert got.tobytes() == np.zeros_like(got).tobytes()
    far = dict(c, halfspaces=None, moving_affine=(np.eye(2), np.array([500.0, -500.0])))
    assert not match(far).any()


def test_fixed_view_as_a_strided_device_window_gives_the_same_bits(hip_device):
    c = nc.match_case(3, "u16")
    host = match(c)
    dev = match(c, fixed=DeviceArray.from_host(c["fixed"]), moving=DeviceArray.from_host(c["moving"]))
    pad = [(2, 1), (3, 2), (5, 4)]
    window = tuple(slice(lo, lo + s) for (lo, _), s in zip(pad, c["fixed"].shape))
    big = DeviceArray.from_host(np.pad(c["fixed"], pad, constant_values=7))
    assert not big[window].is_contiguous()
    strided = match(c, fixed=big[window])
    assert host.tobytes() == dev.tobytes() == strided.tobytes() and host[..., 0].sum() > 500


# ---- independence ---------------------------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_other_blocks_of_the_call(hip_device):
    c = nc.match_case(3, "f32")
    full = match(c)
    subset = [1, 5, 6, 17, len(c["blocks"]) - 1]
    assert np.array_equal(match(c, blocks=c["blocks"][subset]), full[subset], equal_nan=True)
    assert match(c).tobytes() == full.tobytes()                         # equal inputs, equal bits
    assert match(c, batch=5).tobytes() == full.tobytes() and len(c["blocks"]) % 5 != 0      # a call that crosses the wrapper's batch
    assert match(c, batch=1).tobytes() == full.tobytes()


@pytest.mark.parametrize("dtype_name", ["u16", "f32"])
@pytest.mark.parametrize("ndim", [2, 3])
def test_one_block_at_radius_zero_is_pair_moments_of_its_box(hip_device, ndim, dtype_name):
    """mvs_block_match against mvs_pair_moments, as test_rows_partition_the_samples_of_the_pair of tests/test_intensity_gpu.py ties
    mvs_intensity_pair_moments to it: the largest block at the grid's origin that fits the kernel, radius 0, against the grid of the
    block's shape.  A voxel that one of the two drops shows in n; the rest are double sums of at most 1e5 terms merged in
    different trees, 1e-9 relative (the oracles agree within that: tests/test_nonrigid_host.py)."""
    c = nc.match_case(ndim, dtype_name)
    block = nc.largest_block(c["grid_shape"])
    n = tuple(int(v) for v in block[0, 1])
    got = _nonrigid_ops.block_match(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], block, (0,) * ndim, c["halfspaces"])
    assert got.shape == (1, 1, 6)
    row = got[0, 0]
    whole = _metric_ops.pair_moments(c["fixed"], c["moving"], c["fixed_affine"], [c["moving_affine"]], n, c["halfspaces"])[0]
    print("block", n, "row", row, "whole", whole)
    assert row[0] == whole[0] and whole[0] > 500
    np.testing.assert_allclose(row[1:3], whole[1:3], rtol=1e-9)
    np.testing.assert_allclose(row[3:], whole[3:], rtol=1e-9, atol=1e-9 * max(whole[3], whole[4]))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip_device):
    c = nc.match_case(3, "u16")
    with pytest.raises(_lib.MvsError, match="exceed") as e:            # 30^3 + 36^3 samples
        _nonrigid_ops.block_match(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], np.array([[[0, 0, 0], [30, 30, 30]]]), (3, 3, 3))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    fits = np.array([[[0, 0, 0], [4, 4, 4]]])
    assert _nonrigid_ops.block_match(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], fits, (8, 8, 8)).shape == (1, 17 ** 3, 6)
    with pytest.raises(_lib.MvsError, match="radius") as e:
        _nonrigid_ops.block_match(c["fixed"], c["moving"], c["fixed_affine"], c["moving_affine"], fits, (2, 9, 2))
    assert e.value.code == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.MvsError, match="share one dtype") as e:
        match(c, moving=nc.match_case(3, "u8")["moving"])
    assert e.value.code == _lib.ERR_UNSUPPORTED
    x = DeviceArray.from_host(c["fixed"])
    before = x.get()
    field = np.zeros((1, 1, 1, 3), np.float32)
    with pytest.raises(_lib.MvsError, match="overlaps") as e:          # the kernel gathers: never in place
        _nonrigid_ops.warp_field(x, field, out=x)
    assert e.value.code == -1                                           # MVS_ERR_INVALID_ARG
    big = DeviceArray.from_host(np.zeros((44, 48, 56), np.uint16))
    with pytest.raises((_lib.MvsError, ValueError)):                    # an output that starts inside the input's window
        _nonrigid_ops.warp_field(big[2:42], field, out=big[4:44])
    assert same_bits(x.get(), before)
    with pytest.raises(ValueError, match="finite"):
        _nonrigid_ops.warp_field(c["fixed"], np.full((1, 1, 1, 3), np.nan, np.float32))


# ---- warp -----------------------------------------------------------------------------------------------------------------------------
WARP_CASES = [((24, 40, 72), (1, 2, 5)), ((24, 40, 72), (3, 3, 3)), ((40, 130), (2, 7))]


def warp_field_of(nodes, seed):
    """Displacements of up to +-3 px; along every axis the first cells push below 0 and the last ones past n - 1 (an axis with one
    cell pushes past one of its borders)."""
    field = np.random.default_rng(seed).uniform(-3.0, 3.0, tuple(nodes) + (len(nodes),)).astype(np.float32)
    for ax, g in enumerate(nodes):
        if g > 1:
            first, last = [slice(None)] * len(nodes) + [ax], [slice(None)] * len(nodes) + [ax]
            first[ax], last[ax] = 0, g - 1
            field[tuple(first)] = -np.abs(field[tuple(first)]) * 0.8 - 0.5
            field[tuple(last)] = np.abs(field[tuple(last)]) * 0.8 + 0.5
    assert np.abs(field).max() <= 3.0
    return field


def assert_warp_close(got, want_float, data, out_dtype):
    out_dtype = np.dtype(out_dtype)
    assert got.dtype == out_dtype and got.shape == want_float.shape
    if out_dtype.kind == "f":
        span = float(data.max()) - float(data.min())
        bar = 1e-4 * np.maximum(np.abs(want_float), 1e-3 * span)       # the bar of helpers.fused_close_stats
        err = np.abs(got.astype(np.float64) - want_float)
        print(f"    float32: max err / bar {np.max(err / bar):.3g}")
        assert np.all(err <= bar)
        return
    want = no.to_dtype(want_float, out_dtype)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert diff.max() <= 1
    flips = diff == 1
    frac = want_float - np.floor(want_float)
    near = np.abs(frac - 0.5) <= 1e-4 * np.maximum(np.abs(want_float), 1.0)
    print(f"    {out_dtype}: {int(flips.sum())} flips")
    assert np.all(near[flips])


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape,nodes", WARP_CASES)
def test_warp_matches_the_float64_restatement(hip_device, shape, nodes, dtype_name):
    dtype = DTYPES[dtype_name]
    x = texture(shape, 61 + len(shape), dtype)
    field = warp_field_of(nodes, 7)
    d = no.displacement(shape, field)
    idx = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    for ax, (n, g) in enumerate(zip(shape, nodes)):                     # the clamp works at every border
        under, over = bool((idx[ax] + d[..., ax] < 0).any()), bool((idx[ax] + d[..., ax] > n - 1).any())
        assert (under and over) if g > 1 else (under or over)
    want_float = no.warp_float(x, field)
    pad = [(1, 2), (2, 1), (3, 5)][-len(shape):]
    window = DeviceArray.from_host(np.pad(x, pad, constant_values=3))[tuple(slice(lo, lo + s) for (lo, _), s in zip(pad, shape))]
    assert not window.is_contiguous()
    for out_dtype in dict.fromkeys([dtype, np.float32]):
        host = _nonrigid_ops.warp_field(x, field, out_dtype=out_dtype)
        dev = _nonrigid_ops.warp_field(DeviceArray.from_host(x), field, out_dtype=out_dtype)
        strided = _nonrigid_ops.warp_field(window, field, out_dtype=out_dtype)
        assert isinstance(host, np.ndarray) and isinstance(dev, DeviceArray) and strided.is_contiguous()
        assert_warp_close(host, want_float, x, out_dtype)
        assert same_bits(dev.get(), host) and same_bits(strided.get(), host)
    zero = np.zeros_like(field)
    assert same_bits(_nonrigid_ops.warp_field(x, zero), x) and same_bits(_nonrigid_ops.warp_field(window, zero).get(), x)
    if dtype != np.float32:
        assert same_bits(_nonrigid_ops.warp_field(x, zero, out_dtype=np.float32), x.astype(np.float32))


def test_warp_rows_off_the_vectors_and_nan_taps(hip_device):
    x = texture((5, 67), 3, np.uint8)                                   # rows of 67 bytes: the 16-byte stores start at another x in every row
    field = warp_field_of((2, 3), 9)
    assert_warp_close(_nonrigid_ops.warp_field(x, field), no.warp_float(x, field), x, np.uint8)
    f = texture((6, 9), 4, np.float32)
    f[2, 4] = np.nan
    half = np.full((1, 1, 2), 0.5, np.float32)
    got = _nonrigid_ops.warp_field(f, half)
    want = no.warp_float(f, half)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 4      # the four voxels whose taps include the NaN
    assert np.array_equal(_nonrigid_ops.warp_field(f, half, out_dtype=np.float32)[~np.isnan(want)], got[~np.isnan(want)])
    as_int = _nonrigid_ops.warp_field(np.full((4, 8), 65535, np.uint16), half)
    assert np.all(as_int == 65535)


# ---- shifts and fields against the oracle, end to end ----------------------------------------------------------------------------------
def fit(name, msims, **kw):
    """fit_fields with the arguments of case ``name`` on the face-neighbour pairs of its mosaic (the oracle's pairs)."""
    f = nc.FIT[name]
    return nonrigid.fit_fields(msims, "stage", nodes=f["nodes"], pairs=nc.mosaic(f["ndim"])["pairs"], block=f["block"], radius=f["radius"],
                               min_ncc=f["min_ncc"], return_info=True, **nc.LAMBDAS, **kw)


@pytest.mark.parametrize("name", list(nc.FIT))
def test_shifts_and_fields_match_the_oracle(hip_device, name):
    m = nc.mosaic(nc.FIT[name]["ndim"])
    want, winfo = nc.oracle_fit(name)
    nc.assert_margins(winfo, min_ncc=nc.FIT[name]["min_ncc"])
    got, info = fit(name, m["msims"])
    assert sorted(info["blocks"]) == sorted(winfo["per_pair"]) == m["pairs"]
    worst = 0.0
    for pair, (blocks, found) in winfo["per_pair"].items():
        g = info["blocks"][pair]
        assert np.array_equal(g["blocks"], blocks)
        assert g["reason"] == [f["reason"] for f in found], pair
        for b, f in enumerate(found):
            if f["reason"] is None:
                worst = max(worst, float(np.abs(g["shift"][b] - f["shift"]).max()))
                assert g["weight"][b] == pytest.approx(f["weight"], rel=1e-6)
        assert info["pairs"][pair]["used"] == sum(1 for f in found if f["reason"] is None)
        assert info["pairs"][pair]["dropped"] == {r: sum(1 for f in found if f["reason"] == r) for r in no.REASONS}
    dfield = max(float(np.abs(a.astype(np.float64) - w).max()) for a, w in zip(got, want))
    print(f"{name}: shifts within {worst:.3g} grid units, fields within {dfield:.3g} px of the oracle's")
    assert worst <= 1e-6 and dfield <= 1e-5
    if name == "2d_tight":
        reasons = [f["reason"] for _, found in winfo["per_pair"].values() for f in found]
        assert "rim" in reasons and "low_ncc" in reasons and None in reasons


# ---- the feature does its job -------------------------------------------------------------------------------------------------------
def weighted_rms(info):
    w = np.array([p["w"] for p in info["pairs"].values() if p["used"]])
    r = np.array([p["rms_before"] for p in info["pairs"].values() if p["used"]])
    return float(np.sqrt(np.sum(w * r ** 2) / np.sum(w)))


@pytest.mark.parametrize("name", ["2d", "3d"])
def test_corrected_tiles_agree_in_their_overlaps(hip_device, name):
    """The weighted RMS of the shifts that block matching finds after the correction over the one before.  With the oracle alone
    (float64 sampling): 0.216 for the 2 x 2 mosaic of 160 x 160 float32 tiles with 4 x 4 cells, 0.610 for the two 48 x 64 x 64
    uint16 tiles with 2 x 2 x 2 cells.  The device path differs in its float32 sampling only: at most the oracle's ratio + 0.05."""
    m = nc.mosaic(nc.FIT[name]["ndim"])
    oracle = nc.oracle_ratio(name)
    assert abs(oracle - {"2d": 0.216, "3d": 0.610}[name]) < 2e-3      # the docstring's figure
    fields, before = fit(name, m["msims"])
    corrected = nonrigid.apply_fields(m["msims"], fields)
    assert all(msi_utils.is_msim(c) and c.transforms.keys() == x.transforms.keys() for c, x in zip(corrected, m["msims"]))
    assert all(c["scale0"].data.dtype == x["scale0"].data.dtype and c["scale0"].data.shape == x["scale0"].data.shape for c, x in zip(corrected, m["msims"]))
    assert all(c["scale0"].dims == x["scale0"].dims for c, x in zip(corrected, m["msims"]))
    _, after = fit(name, corrected)
    ratio = weighted_rms(after) / weighted_rms(before)
    print(f"{name}: residual shift after / before {ratio:.4f} (oracle {oracle:.4f})")
    assert ratio <= oracle + 0.05 and ratio < 1.0
    fused = fusion.fuse([msi_utils.get_sim_from_msim(c) for c in corrected], transform_key="stage")
    raw = fusion.fuse([msi_utils.get_sim_from_msim(x) for x in m["msims"]], transform_key="stage")
    assert fused.data.shape == raw.data.shape and fused.data.dtype == raw.data.dtype
    assert np.abs(np.asarray(fused.data, dtype=np.float64) - np.asarray(raw.data, dtype=np.float64)).max() > 0


def test_apply_fields_keeps_the_kind_of_image(hip_device):
    """Spatial images, resident tiles, a pyramid and a view with two channels (the mosaic's own images carry c and t axes of one)."""
    m = nc.mosaic(2)
    raw = [v["data"] for v in m["views"]]
    fields, _ = fit("2d", m["msims"])
    host = nonrigid.apply_fields(m["msims"], fields)
    want = [_nonrigid_ops.warp_field(x, f) for x, f in zip(raw, fields)]
    assert all(same_bits(np.squeeze(np.asarray(h["scale0"].data)), w) for h, w in zip(host, want))
    sims = [msi_utils.get_sim_from_msim(x) for x in m["msims"]]
    as_sims = nonrigid.apply_fields(sims, fields)
    assert all(not msi_utils.is_msim(s) and s.dims == x.dims and same_bits(np.squeeze(np.asarray(s.data)), w) for s, x, w in zip(as_sims, sims, want))
    resident = nonrigid.apply_fields([to_device(s) for s in sims], fields, out_dtype=np.float32)
    assert all(isinstance(r.data, DeviceArray) and same_bits(np.squeeze(r.data.get()), w) for r, w in zip(resident, want))
    refit, _ = fit("2d", [msi_utils.get_msim_from_sim(to_device(s)) for s in sims])
    assert all(same_bits(a, b) for a, b in zip(refit, fields))         # resident tiles are read in place and give the same fields
    # a pyramid: the further levels are rebuilt from the corrected scale0
    pyramid, _ = make_tile(raw[0], {"stage": translation_affine([0.0, 0.0])}, scale_factors=[{"y": 2, "x": 2}])
    out = nonrigid.apply_fields([pyramid], fields[:1])[0]
    assert msi_utils.get_sorted_scale_keys(out) == msi_utils.get_sorted_scale_keys(pyramid) == ["scale0", "scale1"]
    assert same_bits(np.squeeze(np.asarray(out["scale0"].data)), want[0]) and out["scale1"].data.shape == pyramid["scale1"].data.shape
    # two channels: every channel goes through the kernel with the view's field; the fit reads channel_index
    second = [np.ascontiguousarray(x[::-1]) for x in raw]
    with_c = [make_tile(np.stack([x, y]), {"stage": translation_affine([float(v) for v in o])}, c_coords=["a", "b"])[0]
              for x, y, o in zip(raw, second, m["origins"])]
    fields_c, _ = fit("2d", with_c, channel_index=0)
    assert all(same_bits(a, b) for a, b in zip(fields_c, fields))
    other, _ = fit("2d", with_c, channel_index=1)
    assert not all(same_bits(a, b) for a, b in zip(other, fields))
    warped = np.squeeze(np.asarray(nonrigid.apply_fields(with_c[:1], fields[:1])[0]["scale0"].data))
    assert warped.shape == (2,) + raw[0].shape and same_bits(warped[0], want[0])
    assert same_bits(warped[1], _nonrigid_ops.warp_field(second[0], fields[0]))
    with pytest.raises(ValueError, match="one field per view"):
        nonrigid.apply_fields(m["msims"], fields[:2])
    with pytest.raises(ValueError, match="lambda_identity"):
        nonrigid.fit_fields(m["msims"], "stage", lambda_identity=0.0)
    # without ``pairs`` the overlapping pairs of the view adjacency graph are used: the four faces and the two diagonals
    _, info = nonrigid.fit_fields(m["msims"], "stage", return_info=True)
    assert sorted(info["pairs"]) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
