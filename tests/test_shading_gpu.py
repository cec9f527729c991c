"""GPU tests of the shading correction: mvs_stack_quantiles against the sort-based restatement of tests/shading_oracle.py (a
selection: every plane and every count equal), mvs_plane_apply bit for bit against the numpy float32 restatement, and
estimate_shading / apply_shading end to end on a planted profile.

Shapes are the smallest that reach every path: rows shorter than, equal to and one past a strip of 32 / 64 / 128 pixels and several
strips long, fewer planes than the 32 half waves of a workgroup and more, rows that are and are not 4-byte aligned; for the apply
kernel rows below, at and off its 16-byte vectors, slabs of one plane and of several, plane pitches that keep and break the
vectors' alignment."""
import functools

import numpy as np
import pytest

from multiview_stitcher_amd import _shading_ops, intensity, msi_utils
from multiview_stitcher_amd.device import DeviceArray, to_device
from tests import shading_oracle as so
from tests.helpers import apply_coeff, apply_input, same_bits
from tests.shading_helpers import CASES, RECOVERY_CAP, oracle_planes, planted_case, recovery_error

pytestmark = pytest.mark.gpu

DTYPES = {"u8": np.uint8, "u16": np.uint16, "f32": np.float32}
Q5 = (0, 0.02, 0.5, 0.73, 1)


def random_tile(shape, dtype, rng):
    if dtype == np.float32:
        x = (rng.standard_normal(shape) * 50).astype(np.float32)
        x[rng.random(shape) < 0.2] = np.nan
        return x
    return rng.integers(0, np.iinfo(dtype).max + 1, size=shape).astype(dtype)


def assert_selects_like_the_oracle(tiles, q=Q5, got=None):
    """q in calls of at most four quantiles; every plane and the counts equal to the oracle's.  Returns (planes, counts)."""
    want_p, want_c = so.stack_quantiles(tiles, q)
    q = list(q)
    if got is None:
        parts = [_shading_ops.stack_quantiles(tiles, q[i:i + 4]) for i in range(0, len(q), 4)]
        got = np.concatenate([p for p, _ in parts]), parts[0][1]
        assert all(np.array_equal(c, parts[0][1]) for _, c in parts)
    planes, counts = got
    assert planes.dtype == np.float32 and counts.dtype == np.int32 and planes.shape == want_p.shape
    assert np.array_equal(counts, want_c), np.argwhere(counts != want_c)[:5]
    same = (planes == want_p) | (np.isnan(planes) & np.isnan(want_p))
    assert same.all(), (np.argwhere(~same)[:5], planes[~same][:5], want_p[~same][:5])
    return planes, counts


def same_planes(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


# ---- quantiles against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_quantiles_of_2d_tiles(hip_device, dtype_name):
    rng = np.random.default_rng(11)
    tiles = [random_tile((3, 70), DTYPES[dtype_name], rng) for _ in range(37)]      # 37 planes: more than one step of the half waves
    assert_selects_like_the_oracle(tiles)


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_quantiles_of_3d_views_of_different_depth(hip_device, dtype_name):
    rng = np.random.default_rng(12)
    tiles = [random_tile((z, 24, 70), DTYPES[dtype_name], rng) for z in (3, 7, 4, 1, 6)]
    planes, counts = assert_selects_like_the_oracle(tiles)
    if dtype_name != "f32":
        assert (counts == 21).all()
        stack = so.stack_of(tiles)
        assert np.array_equal(planes[0], stack.min(axis=0)) and np.array_equal(planes[4], stack.max(axis=0))


@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", [5, 63, 64, 65, 130, 257])
def test_quantiles_at_the_strip_edges(hip_device, w, h):
    """Widths that straddle any strip width from 32 to 256; 1, 2 and 9 views; 1 and 2 planes (fewer than half waves) and 45."""
    rng = np.random.default_rng(100 * w + h)
    for dtype in DTYPES.values():
        for zs in ((1,), (1, 1), (5,) * 9):
            assert_selects_like_the_oracle([random_tile((z, h, w), dtype, rng) for z in zs], q=(0.02, 0.5, 1))


def test_quantiles_of_hard_uint16_values(hip_device):
    rng = np.random.default_rng(13)
    shape = (40, 3, 70)
    one_high_digit = (0x1200 + rng.integers(0, 256, size=shape)).astype(np.uint16)           # all within 0x1200 .. 0x12FF
    only_high_digit = (rng.integers(0, 256, size=shape) << 8).astype(np.uint16)              # k << 8
    constant = np.full(shape, 0x1234, np.uint16)
    eight_bit = rng.integers(0, 6, size=shape).astype(np.uint16)                              # heavy ties
    for stack in (one_high_digit, only_high_digit, constant, eight_bit):
        assert_selects_like_the_oracle([stack[:17], stack[17:]])
    planes, _ = _shading_ops.stack_quantiles([constant], Q5[:4])
    assert (planes == 0x1234).all()


def test_quantiles_of_hard_float_values(hip_device):
    rng = np.random.default_rng(14)
    shape = (50, 3, 70)
    x = (rng.standard_normal(shape) * 4).astype(np.float32)
    pick = rng.integers(0, 10, size=shape)
    x[pick == 0] = -0.0
    x[pick == 1] = 0.0
    x[pick == 2] = np.inf
    x[pick == 3] = -np.inf
    x[pick == 4] = np.float32(1e-41) * rng.choice(np.float32([-3, -1, 1, 2]), size=shape)[pick == 4]     # denormals
    x[rng.random(shape) < 0.2] = np.nan
    x[:, 1, 7] = np.nan                                                                                  # no sample at all
    x[:, 2, 9] = np.nan
    x[31, 2, 9] = -7.25                                                                                  # a single sample
    assert np.signbit(x[np.nonzero(x == 0)]).any() and (np.abs(x[np.isfinite(x) & (x != 0)]) < 1e-38).any()
    planes, counts = assert_selects_like_the_oracle([x[:20], x[20:]])
    assert counts[1, 7] == 0 and np.isnan(planes[:, 1, 7]).all()
    assert counts[2, 9] == 1 and (planes[:, 2, 9] == np.float32(-7.25)).all()
    assert not np.signbit(planes[planes == 0]).any()                                                    # -0 counts as +0
    assert np.isinf(planes[0]).any() and np.isinf(planes[4]).any()


def test_a_bin_holds_more_than_65535_samples(hip_device):
    """One uint8 view of 70 000 planes with 69 000 equal values per pixel: a 16-bit counter would wrap."""
    rng = np.random.default_rng(15)
    x = rng.integers(0, 256, size=(70000, 2, 64)).astype(np.uint8)
    x[500:69500] = 77
    planes, counts = assert_selects_like_the_oracle([x], q=(0, 0.5, 0.995, 1))
    assert (counts == 70000).all() and (planes[1] == 77).all()


# ---- the same bits whatever the order and the memory ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bits_case(dtype_name):
    rng = np.random.default_rng(16)
    return [random_tile((z, 5, 70), DTYPES[dtype_name], rng) for z in (4, 9, 2, 40)]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_view_order_and_memory_do_not_change_the_bits(hip_device, dtype_name):
    tiles = bits_case(dtype_name)
    q = (0.02, 0.5, 0.73)
    first = assert_selects_like_the_oracle(tiles, q)
    assert same_planes(first, _shading_ops.stack_quantiles(tiles[::-1], q))
    resident = [DeviceArray.from_host(t) for t in tiles]
    assert same_planes(first, _shading_ops.stack_quantiles(resident, q))
    assert same_planes(first, _shading_ops.stack_quantiles([resident[0], tiles[1], resident[2], tiles[3]], q))
    # windows at x offset 3 / y offset 1 of larger arrays: rows that are not 4-byte aligned for uint8 / uint16
    big = [np.full((t.shape[0] + 1, t.shape[1] + 2, t.shape[2] + 5), 9, t.dtype) for t in tiles]
    win = (slice(None, -1), slice(1, 6), slice(3, 73))
    for b, t in zip(big, tiles):
        b[win] = t
    dev_windows = [DeviceArray.from_host(b)[win] for b in big]
    assert not dev_windows[0].is_contiguous()
    assert same_planes(first, _shading_ops.stack_quantiles(dev_windows, q))
    host_windows = [b[win] for b in big]
    assert not host_windows[0].flags.c_contiguous
    assert same_planes(first, _shading_ops.stack_quantiles(host_windows, q))


@pytest.mark.parametrize("dtype_name", ["u16", "f32"])
def test_every_second_plane_by_stride(hip_device, dtype_name):
    tiles = bits_case(dtype_name)
    copied = [np.ascontiguousarray(t[::2]) for t in tiles]
    want = assert_selects_like_the_oracle(copied, (0.5,))
    assert same_planes(want, _shading_ops.stack_quantiles([_shading_ops.every_kth_plane(t, 2) for t in tiles], 0.5))
    resident = [_shading_ops.every_kth_plane(DeviceArray.from_host(t), 2) for t in tiles]
    assert [r.shape for r in resident] == [c.shape for c in copied]
    assert same_planes(want, _shading_ops.stack_quantiles(resident, 0.5))


def test_bad_stacks_are_refused(hip_device):
    a = np.zeros((2, 4, 6), np.uint16)
    with pytest.raises(ValueError):
        _shading_ops.stack_quantiles([a, np.zeros((2, 4, 7), np.uint16)], 0.5)
    with pytest.raises(ValueError):
        _shading_ops.stack_quantiles([a, a.astype(np.float32)], 0.5)
    with pytest.raises(ValueError):
        _shading_ops.stack_quantiles([a], [0.1, 0.2, 0.3, 0.4, 0.5])
    with pytest.raises(ValueError):
        _shading_ops.stack_quantiles([a], 1.5)


# ---- apply -----------------------------------------------------------------------------------------------------------------------------
APPLY_SHAPES = [
    # rows of 5, 8, 13, 67; 2-D, z = 1, 2, 9
    (6, 5), (9, 8), (7, 13), (5, 67), (1, 6, 5), (2, 3, 8), (9, 4, 13), (9, 5, 67), (2, 7, 64),
    # slabs of several planes (more than 1024 rows): pitches that keep the 16-byte vectors (8-pixel rows) and that break them
    (40, 1100, 8), (9, 1100, 13),
]


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("shape", APPLY_SHAPES)
def test_apply_matches_the_float32_restatement(hip_device, shape, dtype_name):
    dtype = DTYPES[dtype_name]
    x = apply_input(shape, dtype, 5)
    coeff = apply_coeff(shape[-2:], dtype, 6)
    coeff_dev = DeviceArray.from_host(coeff)
    for out_dtype in dict.fromkeys([dtype, np.float32]):
        want = so.apply(x, coeff, out_dtype)
        if np.dtype(out_dtype).kind != "f":
            hi = np.iinfo(out_dtype).max
            assert (want == 0).any() and (want == hi).any() and ((want > 0) & (want < hi)).any()      # both ends saturate
        host = _shading_ops.apply_plane(x, coeff, out_dtype=out_dtype)
        dev = _shading_ops.apply_plane(DeviceArray.from_host(x), coeff, out_dtype=out_dtype)
        assert isinstance(host, np.ndarray) and isinstance(dev, DeviceArray)
        assert same_bits(host, want), (out_dtype, np.argwhere(host != want)[:5])
        assert same_bits(dev.get(), want)
        # coefficients from device memory, for host and resident tiles
        assert same_bits(_shading_ops.apply_plane(x, coeff_dev, out_dtype=out_dtype), want)
        assert same_bits(_shading_ops.apply_plane(DeviceArray.from_host(x), coeff_dev, out_dtype=out_dtype).get(), want)
    # in place equals out of place, on the device and on the host
    d = DeviceArray.from_host(x)
    assert _shading_ops.apply_plane(d, coeff_dev, out=d) is d and same_bits(d.get(), so.apply(x, coeff))
    h = x.copy()
    _shading_ops.apply_plane(h, coeff, out=h)
    assert same_bits(h, so.apply(x, coeff))


@pytest.mark.parametrize("dtype_name", list(DTYPES))
def test_apply_reads_a_window_at_an_odd_offset(hip_device, dtype_name):
    dtype = DTYPES[dtype_name]
    big = apply_input((10, 12, 80), dtype, 8)
    win = (slice(1, 10), slice(2, 11), slice(3, 70))                    # rows of 67 that start at x = 3
    coeff = apply_coeff((9, 67), dtype, 9)
    window = DeviceArray.from_host(big)[win]
    assert not window.is_contiguous()
    for out_dtype in dict.fromkeys([dtype, np.float32]):
        got = _shading_ops.apply_plane(window, coeff, out_dtype=out_dtype)
        assert got.is_contiguous() and same_bits(got.get(), so.apply(np.ascontiguousarray(big[win]), coeff, out_dtype))


def test_apply_rounds_ties_to_even_and_keeps_nan(hip_device):
    x16 = np.arange(0, 64, dtype=np.uint16).reshape(4, 16)
    half = np.zeros((4, 16, 2), np.float32)
    half[..., 0] = 0.5
    got = _shading_ops.apply_plane(x16, half)
    assert np.array_equal(got, np.rint(x16 * 0.5).astype(np.uint16)) and got[0, 1] == 0 and got[0, 3] == 2 and got[0, 5] == 2
    x8 = np.arange(0, 256, dtype=np.uint8).reshape(8, 32)
    up = np.zeros((8, 32, 2), np.float32)
    up[..., 0], up[..., 1] = 1.0, 0.5                                   # x + 0.5: every value is a tie; 255.5 saturates
    got8 = _shading_ops.apply_plane(x8, up)
    assert np.array_equal(got8, np.minimum(np.rint(x8.astype(np.float32) + 0.5), 255).astype(np.uint8)) and got8[-1, -1] == 255 and got8[0, 0] == 0
    f = np.array([[1.0, np.nan, -2.0, np.inf, 3.0]], np.float32)
    c = np.zeros((1, 5, 2), np.float32)
    c[..., 0], c[..., 1] = 2.0, 1.0
    gotf = _shading_ops.apply_plane(f, c)
    assert np.isnan(gotf[0, 1]) and np.array_equal(gotf[0, [0, 2, 4]], np.float32([3.0, -3.0, 7.0])) and gotf[0, 3] == np.inf
    nan16 = _shading_ops.apply_plane(np.uint16([[5, 6]]), np.float32([[[np.nan, 0.0], [1.0, np.nan]]]))
    assert np.array_equal(nan16, np.uint16([[0, 0]]))                   # a NaN is stored as 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def resident_msims(msims):
    return [msi_utils.get_msim_from_sim(to_device(msi_utils.get_sim_from_msim(m))) for m in msims]


@pytest.mark.parametrize("dtype_name", ["f32", "u16"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_planted_profile_is_estimated_and_removed(hip_device, name, dtype_name):
    """estimate_shading equals shading_from_planes of the oracle's planes exactly (the planes are a selection, the host code is
    shared); the corrected tiles match (I - D0) / F0 + mean(D0) within 0.05 / (1 - 0.05) relative -- what a flat field within
    RECOVERY_CAP of the planted one gives -- plus one count for uint16 tiles.  Without the correction they are off by up to 43 %."""
    case = planted_case(name, dtype_name)
    planes, counts = oracle_planes(name, dtype_name)
    want = intensity.shading_from_planes(planes, counts, darkfield=case["dark"])
    assert recovery_error(want, case) <= RECOVERY_CAP
    bound = RECOVERY_CAP / (1.0 - RECOVERY_CAP)
    extra = 1.0 if dtype_name == "u16" else 0.0
    for msims in (case["msims"], resident_msims(case["msims"])):
        got, info = intensity.estimate_shading(msims, darkfield=case["dark"], return_info=True)
        assert np.array_equal(info["planes"], planes) and np.array_equal(info["counts"], counts)
        assert same_bits(got["flatfield"], want["flatfield"]) and same_bits(got["darkfield"], want["darkfield"]) and got["offset"] == want["offset"]
        corrected = intensity.apply_shading(msims, got, out_dtype=None)
        assert all(msi_utils.is_msim(c) for c in corrected)
        worst = raw_worst = 0.0
        for c, m, clean in zip(corrected, case["msims"], case["clean"]):
            out = np.asarray(msi_utils.get_sim_from_msim(c).data).astype(np.float64).reshape(clean.shape)      # (singleton c / t dims)
            raw = np.asarray(msi_utils.get_sim_from_msim(m).data).astype(np.float64).reshape(clean.shape)
            worst = max(worst, float(((np.abs(out - clean) - extra) / clean).max()))
            raw_worst = max(raw_worst, float((np.abs(raw - clean) / clean).max()))
        print(f"{name} {dtype_name}: corrected tiles within {worst:.4f} relative of the clean ones (bound {bound:.4f}); uncorrected {raw_worst:.3f}")
        assert worst <= bound and raw_worst > 0.3


def test_shading_per_channel_in_place_and_every_second_plane(hip_device):
    """c / t dims: the stack is channel ``channel_index`` of every time point; a dict of models corrects each channel with its own
    plane, in place on resident tiles."""
    from tests.metrics_helpers import make_tile, translation_affine

    rng = np.random.default_rng(21)
    tiles = [rng.integers(100, 4000, size=(2, 6, 9, 20)).astype(np.uint16) for _ in range(3)]           # (c, z, y, x)
    msims = [make_tile(t, {"stage": translation_affine([0.0, 0.0, 0.0])}, c_coords=["a", "b"])[0] for t in tiles]
    got, info = intensity.estimate_shading(msims, channel_index=1, plane_step=2, degree=None, min_samples=1, return_info=True)
    want_p, want_c = so.stack_quantiles([t[1, ::2] for t in tiles], [0.5])
    assert np.array_equal(info["planes"], want_p) and np.array_equal(info["counts"], want_c) and (want_c == 9).all()
    other = {"flatfield": np.full((9, 20), 2.0, np.float32), "darkfield": np.full((9, 20), 50.0, np.float32), "offset": 50.0}
    models = {"a": other, "b": got}
    resident = resident_msims(msims)
    out = intensity.apply_shading(resident, models, inplace=True)
    for o, r, t in zip(out, resident, tiles):
        sim = msi_utils.get_sim_from_msim(o)
        assert sim.data is msi_utils.get_sim_from_msim(r).data
        for ch, key in enumerate("ab"):
            lead = tuple(ch if d == "c" else 0 for d in sim.dims[:2])
            assert same_bits(sim.data[lead].get(), so.apply(t[ch], so.coefficients(models[key])))
