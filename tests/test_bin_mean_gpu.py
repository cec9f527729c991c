"""GPU: every block-mean binning kernel against numpy's ``a[trim].reshape(...).mean(axis=...).astype(dtype)`` in float64, at the edges
of the conditions that pick a kernel (csrc/mvs_bin.hip bin_mean_impl / mvs_bin_mean_batch_async, csrc/mvs_fuse.hip crop_bin_kernel):

  bin_mean_kernel<T>             the generic kernel: any dtype, bins, stride, alignment
  bin_mean_u16x2_kernel          uint16, bin 2 along x, binned width % 4 == 0, y / z strides % 8 == 0, input 16-byte and output 8-byte
                                 aligned, bz * by <= 16384 (32-bit sums)
  bin_mean_u16x2_batch_kernel    the same for up to 32 views per launch; one view that fails a condition sends the WHOLE batch to the
                                 per-view path
  crop_bin_kernel<TIn>           binning inside the crop of the batched pair path: 16-bit, bin 2 along x, 4-byte aligned pairs -> a group
                                 of 8 outputs from 16-byte loads, or (group over the edge of the window) 4-byte pair loads; else generic

Integer results are compared exactly, float32 at rtol 1e-6.  A block whose sum is an exact multiple of its count is where
``sum * (1 / count)`` and a truncating cast give one less than numpy (first at count 49): the exact-multiple cases cover that."""
import ctypes as C

import numpy as np
import pytest
from scipy import ndimage

pytestmark = pytest.mark.gpu

SENTINEL = {np.dtype(np.uint16): 0xABCD, np.dtype(np.uint8): 0xAB, np.dtype(np.float32): -7.5}


def _numpy_bin(a, bins):
    """a[trim].reshape(...).mean(axis=...).astype(dtype), the mean in float64."""
    sl = tuple(slice(0, (n // b) * b) for n, b in zip(a.shape, bins))
    shp = [q for n, b in zip(a.shape, bins) for q in (n // b, b)]
    return a[sl].reshape(shp).mean(axis=tuple(range(1, 2 * a.ndim, 2)), dtype=np.float64).astype(a.dtype)


def _block_sums(a, bins):
    """The exact sum of every block (float64 holds them: < 2^53)."""
    sl = tuple(slice(0, (n // b) * b) for n, b in zip(a.shape, bins))
    shp = [q for n, b in zip(a.shape, bins) for q in (n // b, b)]
    return a[sl].astype(np.float64).reshape(shp).sum(axis=tuple(range(1, 2 * a.ndim, 2)))


def _assert_binned(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if want.dtype == np.float32:
        np.testing.assert_allclose(got, want, rtol=1e-6)
    else:
        np.testing.assert_array_equal(got, want)


def _check(a, bins):
    """bin_mean of the host array and of its contiguous device copy against numpy."""
    from multiview_stitcher_amd import _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    want = _numpy_bin(a, bins)
    _assert_binned(_reg_ops.bin_mean(a, list(bins)), want)
    _assert_binned(_reg_ops.bin_mean(DeviceArray.from_host(a, 0), list(bins)).get(), want)
    return want


def _random(rng, shape, dtype):
    if dtype == np.float32:
        return (rng.random(shape) * 4000).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max, shape, dtype=dtype, endpoint=True)


# ---- exact multiples ------------------------------------------------------------------------------------------------------------------
def _block_values(n, dtype):
    """n block means: every small one (1, 2, 3, 4, 6, 7, 8 are the first that sum * (1 / 49) truncates to one less), the largest,
    and a seeded sample of the rest."""
    top = np.iinfo(dtype).max
    rng = np.random.default_rng(n)
    v = np.concatenate([np.arange(min(n // 2, top + 1)), [top, top - 1, top // 2 + 1], rng.integers(0, top, n, endpoint=True)])[:n]
    return v.astype(dtype)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["u16", "u8"])
@pytest.mark.parametrize("bins,grid", [((7, 7), (24, 40)), ((2, 7, 7), (3, 10, 32)), ((1, 103, 1), (3, 4, 200)), ((7, 7, 2), (2, 12, 40))], ids=str)
def test_constant_blocks_bin_to_their_value(hip_device, dtype, bins, grid):
    """Tiles made of constant blocks (sum = value * count exactly; counts 49, 98, 103, 98) plus a trimmed remainder of b - 1 voxels on
    every axis.  (7, 7) [a 2D tile: bins (1, 7, 7)], (2, 7, 7), (1, 103, 1): bx != 2 -> bin_mean_kernel<T>.  (7, 7, 2): no remainder
    along x, so the rows are 80 elements (% 8 == 0) and the binned width is 40 (% 4 == 0) -> bin_mean_u16x2_kernel for uint16,
    bin_mean_kernel<uint8> for uint8."""
    values = _block_values(int(np.prod(grid)), dtype).reshape(grid)
    a = values
    for axis, b in enumerate(bins):
        a = np.repeat(a, b, axis=axis)
    pad = [(0, b - 1) for b in bins]
    if bins[-1] == 2:
        pad[-1] = (0, 0)
    a = np.pad(a, pad, mode="constant", constant_values=5)
    want = _check(np.ascontiguousarray(a), bins)
    np.testing.assert_array_equal(want, values)


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["u16", "u8"])
@pytest.mark.parametrize("bins,shape", [((7, 7), (170, 285)), ((2, 7, 7), (7, 72, 227)), ((1, 103, 1), (3, 415, 200)), ((7, 7, 2), (15, 85, 80))], ids=str)
def test_few_grey_levels(hip_device, dtype, bins, shape):
    """Tiles of few grey levels, where block sums hit multiples of the count by chance and by construction: (a) voxels drawn from the
    levels 0..2, (b) from {0, 1, 2} * count, so that EVERY block sum is a multiple of the count (means 0 .. 2 * count).  Kernels as in
    test_constant_blocks_bin_to_their_value: bin_mean_kernel<T>, and bin_mean_u16x2_kernel for uint16 with bins (7, 7, 2) (binned
    width 40, stride 80)."""
    rng = np.random.default_rng(11)
    count = int(np.prod(bins))
    a = rng.integers(0, 3, shape).astype(dtype)
    _check(a, bins)
    assert np.count_nonzero(_block_sums(a, bins) == count) >= 10             # (block sums scatter around 1 * count: some hit it)
    b = (rng.integers(0, 3, shape) * count).astype(dtype)                    # (2 * 103 = 206 fits uint8)
    want = _check(b, bins)
    np.testing.assert_array_equal(want * float(count), _block_sums(b, bins))  # every mean is a whole number
    assert want.max() > count


# ---- the vector kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins,shape", [((2, 2, 2), (10, 22, 72)), ((3, 5, 2), (10, 22, 72)), ((2, 2), (44, 136))], ids=str)
@pytest.mark.parametrize("fill", ["random", "saturated"])
def test_vector_kernel_random_and_saturated(hip_device, bins, shape, fill):
    """uint16, bx = 2, binned widths 36 and 68 (% 4 == 0), contiguous rows of 72 / 136 elements (% 8 == 0), fresh allocations ->
    bin_mean_u16x2_kernel, with trimmed remainders along z and y (10 = 3 * 3 + 1, 22 = 5 * 4 + 2), more than one block of 256 threads
    ((2, 2, 2): 5 * 11 * 9 = 495 groups) and all-65535 input (every sum = 65535 * count, the largest a block can have)."""
    a = _random(np.random.default_rng(2), shape, np.uint16) if fill == "random" else np.full(shape, 65535, np.uint16)
    want = _check(a, bins)
    if fill == "saturated":
        assert np.all(want == 65535)


@pytest.mark.parametrize("by,kernel", [(128, "vector"), (129, "generic")])
def test_accumulator_limit_of_the_vector_kernel(hip_device, by, kernel):
    """bz * by = 128 * 128 = 16384 on a (128, 128, 8) uint16 tile: the last product bin_mean_impl gives to bin_mean_u16x2_kernel (binned
    width 4, stride 8); saturated input makes its 32-bit sums 2 * 16384 * 65535 = 2147450880, the stated limit.  bz * by = 128 * 129 =
    16512 on (128, 129, 8): over the limit -> bin_mean_kernel<uint16> (double sums).  Saturated, random and constant-block content."""
    shape, bins = (128, by, 8), (128, by, 2)
    assert (bins[0] * bins[1] <= 16384) == (kernel == "vector")
    rng = np.random.default_rng(by)
    want = _check(np.full(shape, 65535, np.uint16), bins)
    assert want.shape == (1, 1, 4) and np.all(want == 65535)
    _check(_random(rng, shape, np.uint16), bins)
    values = np.array([1, 7, 40000, 65534], np.uint16)
    want = _check(np.ascontiguousarray(np.broadcast_to(np.repeat(values, 2), shape)), bins)
    np.testing.assert_array_equal(want.ravel(), values)


# ---- conditions that leave the vector kernel, one each ----------------------------------------------------------------------------------
WINDOWS = {
    # name: (allocation shape, window, kernel a uint16 window takes with bins (2, 2, 2))
    "binned_width_not_multiple_of_4": ((6, 10, 20), (slice(None), slice(None), slice(None)), "generic"),       # ox = 10
    "odd_y_stride": ((6, 10, 41), (slice(None), slice(None), slice(0, 40)), "generic"),                        # sy = 41, sz = 410
    "x_start_not_multiple_of_8": ((6, 10, 48), (slice(None), slice(None), slice(4, 44)), "generic"),           # pointer + 8 bytes
    "x_start_multiple_of_8_strided": ((8, 12, 64), (slice(1, 7), slice(2, 12), slice(8, 48)), "vector"),       # + 1808 bytes, sy 64, sz 768
}


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8, np.float32], ids=["u16", "u8", "f32"])
@pytest.mark.parametrize("name", list(WINDOWS))
def test_device_windows(hip_device, name, dtype):
    """Windows cut from a DeviceArray (zero-copy: pointer + strides), bins (2, 2, 2), window shape (6, 10, 40) -> binned width 20 (% 4
    == 0) except in the first case.  uint16: each of the first three cases breaks exactly one condition of bin_mean_u16x2_kernel (binned
    width 10; y stride 41; pointer 8 bytes past a 16-byte boundary) -> bin_mean_kernel<uint16>; the fourth keeps them all (window
    starts 1 * 768 + 2 * 64 + 8 = 904 elements = 1808 bytes = 113 * 16 into the allocation, strides 64 and 768) and stays on
    bin_mean_u16x2_kernel with non-contiguous rows and planes.  uint8 / float32: bin_mean_kernel<T> on the same strided windows."""
    from multiview_stitcher_amd import _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    alloc, window, kernel = WINDOWS[name]
    a = _random(np.random.default_rng(len(name)), alloc, dtype)
    d = DeviceArray.from_host(a, 0)
    win = d[window]
    if name != "binned_width_not_multiple_of_4":
        assert not win.is_contiguous() and win.shape == (6, 10, 40)
    if dtype == np.uint16:
        vec = (win.shape[2] // 2) % 4 == 0 and win.strides[0] % 8 == 0 and win.strides[1] % 8 == 0 and win.ptr % 16 == 0
        assert vec == (kernel == "vector")           # (the conditions of bin_mean_impl, restated on this window)
    _assert_binned(_reg_ops.bin_mean(win, [2, 2, 2]).get(), _numpy_bin(a[window], (2, 2, 2)))
    np.testing.assert_array_equal(d.get(), a)        # the input allocation is only read


# ---- out= and wait=False ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
@pytest.mark.parametrize("wait", [True, False])
def test_out_argument_and_unwaited_call(hip_device, dtype, wait):
    """_reg_ops.bin_mean(out=..., wait=...): the result lands in the given array (planes 1..5 of a larger allocation whose first and
    last planes must keep their fill), with the final wait (mvs_bin_mean) and without (mvs_bin_mean_async + _lib.synchronize).
    (10, 22, 72) with bins (2, 2, 2): uint16 -> bin_mean_u16x2_kernel (out pointer = one plane of 11 * 36 * 2 = 792 bytes into the
    allocation, % 8 == 0), float32 -> bin_mean_kernel<float>."""
    from multiview_stitcher_amd import _lib, _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    a = _random(np.random.default_rng(6), (10, 22, 72), dtype)
    want = _numpy_bin(a, (2, 2, 2))
    host = np.full((7, 11, 36), SENTINEL[np.dtype(dtype)], dtype)
    big = DeviceArray.from_host(host, 0)
    out = big[1:6]
    assert out.is_contiguous() and out.ptr % 8 == 0
    got = _reg_ops.bin_mean(DeviceArray.from_host(a, 0), [2, 2, 2], wait=wait, out=out)
    assert got is out
    if not wait:
        _lib.synchronize(0)
    whole = big.get()
    _assert_binned(whole[1:6], want)
    np.testing.assert_array_equal(whole[[0, 6]], host[[0, 6]])
    with pytest.raises(ValueError):
        _reg_ops.bin_mean(DeviceArray.from_host(a, 0), [2, 2, 2], out=big[1:5])


# ---- mvs_bin_mean_batch_async -----------------------------------------------------------------------------------------------------------
BATCHES = {
    # name: (views, dtype, view shape, row length of the input allocation, {view: x start}, kernel)
    "35_views": (35, np.uint16, (4, 6, 32), 32, {}, "batch"),                    # launches of 32 and 3 views (table tail clamped to the last)
    "32_views": (32, np.uint16, (4, 6, 32), 32, {}, "batch"),
    "1_view": (1, np.uint16, (4, 6, 32), 32, {}, "batch"),
    "33_views_strided": (33, np.uint16, (4, 6, 32), 40, {}, "batch"),            # rows of 40 (% 8 == 0): still the vector kernel
    "one_view_misaligned": (35, np.uint16, (4, 6, 32), 40, {17: 4}, "per_view"), # view 17 starts 8 bytes past a 16-byte boundary
    "odd_width": (5, np.uint16, (4, 6, 31), 31, {}, "per_view"),                 # 31 // 2 = 15 outputs per row; odd strides
    "uint8": (5, np.uint8, (4, 6, 32), 32, {}, "per_view"),
    "float32": (5, np.float32, (4, 6, 32), 32, {}, "per_view"),
}


@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_entry_point(hip_device, name):
    """mvs_bin_mean_batch_async through ctypes, bins (2, 2, 2), distinct random content per view (a swapped table entry shows).
    "batch" cases meet every condition of the call's vector test for all views -> bin_mean_u16x2_batch_kernel, 32 views per launch
    (35 and 33 views: a second launch whose pointer table repeats its last view in the unused entries); "per_view" cases fail one
    (one pointer % 16 != 0; shape[2] / 2 = 15 not a multiple of 4; dtype) -> the whole batch goes view by view through bin_mean_impl,
    which picks bin_mean_kernel<T> -- or, for the 34 aligned views of "one_view_misaligned", bin_mean_u16x2_kernel.  Every output is
    planes 1..2 of its own 4-plane slot of ONE allocation: the planes before and after each output, the last slot's tail included,
    must keep their fill, as must an allocation made after the outputs, and the inputs are only read."""
    from multiview_stitcher_amd import _lib
    from multiview_stitcher_amd.device import DeviceArray

    n, dtype, shape, row, starts, kernel = BATCHES[name]
    dtype = np.dtype(dtype)
    lib = _lib.init(0)
    a = _random(np.random.default_rng(n), (n, shape[0], shape[1], row), dtype)
    d = DeviceArray.from_host(a, 0)
    oshape = tuple(s // 2 for s in shape)
    host_out = np.full((n, oshape[0] + 2) + oshape[1:], SENTINEL[dtype], dtype)
    out = DeviceArray.from_host(host_out, 0)
    after = DeviceArray.from_host(np.full(4096, SENTINEL[dtype], dtype), 0)      # an allocation made after the outputs
    views = [d[v, :, :, starts.get(v, 0):starts.get(v, 0) + shape[2]] for v in range(n)]
    outs = [out[v, 1:1 + oshape[0]] for v in range(n)]
    strides = views[0].strides
    assert all(w.strides == strides and w.shape == shape for w in views) and all(o.is_contiguous() for o in outs)
    vec = (dtype == np.uint16 and (shape[2] // 2) % 4 == 0 and strides[0] % 8 == 0 and strides[1] % 8 == 0
           and all(w.ptr % 16 == 0 for w in views) and all(o.ptr % 8 == 0 for o in outs))
    assert vec == (kernel == "batch")                # (the conditions of mvs_bin_mean_batch_async, restated on these views)
    ins_p = (C.c_void_p * n)(*[w.ptr for w in views])
    outs_p = (C.c_void_p * n)(*[o.ptr for o in outs])
    rc = lib.mvs_bin_mean_batch_async(0, n, ins_p, _lib.DTYPE_CODES[dtype], _lib.i64x3(shape), _lib.i64x3(strides), _lib.i64x3([2, 2, 2]), outs_p)
    _lib.check(rc, 0, "mvs_bin_mean_batch_async")
    _lib.synchronize(0)
    want = host_out.copy()
    for v in range(n):
        x0 = starts.get(v, 0)
        want[v, 1:1 + oshape[0]] = _numpy_bin(a[v, :, :, x0:x0 + shape[2]], (2, 2, 2))
    got = out.get()
    if dtype == np.float32:
        np.testing.assert_allclose(got, want, rtol=1e-6)
        np.testing.assert_array_equal(got[:, [0, -1]], want[:, [0, -1]])
    else:
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(d.get(), a)
    assert np.all(after.get() == SENTINEL[dtype])


# ---- crop_bin_kernel through mvs_register_pairs -----------------------------------------------------------------------------------------
def _quantised_field(shape, sigma, dtype):
    """A smooth random field in 12 grey levels (uint16: level * 257, both bytes in use; uint8: level * 21): large constant patches, so
    many bins hold one value and their sums are exact multiples of the count."""
    rng = np.random.default_rng(sum(shape))
    f = ndimage.gaussian_filter(rng.random(shape), sigma)
    f = (f - f.min()) / (f.max() - f.min())
    return (np.minimum((f * 12).astype(np.int64), 11) * (257 if np.dtype(dtype) == np.uint16 else 21)).astype(dtype)


def _host_crop(window, bins, t, out_shape):
    """numpy binning of the raw window, then the whole-pixel crop: out[p] = binned[p + t], NaN outside the binned window."""
    binned = _numpy_bin(window, bins).astype(np.float32)
    out = np.full(out_shape, np.nan, np.float32)
    src, dst = [], []
    for n, o, tk in zip(binned.shape, out_shape, t):
        lo, hi = max(0, -tk), min(o, n - tk)
        assert hi > lo
        dst.append(slice(lo, hi))
        src.append(slice(lo + tk, hi + tk))
    out[tuple(dst)] = binned[tuple(src)]
    return out


CROP_WIDTHS = {
    # name: (binned crop width, extra columns of the raw allocation made odd, raw x start of the windows)
    "groups_of_8": (48, False, 0),        # 6 whole groups per row
    "hanging_group": (51, False, 0),      # 7 groups; the last one is moved back to end with the row
    "odd_raw_width": (51, True, 1),       # odd y / z strides and a window that starts at raw x = 1
}


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8], ids=["u16", "u8"])
@pytest.mark.parametrize("bins", [(1, 2, 2), (1, 7, 7), (3, 2, 2)], ids=str)
@pytest.mark.parametrize("width", list(CROP_WIDTHS))
def test_crop_bin_kernel_equals_numpy_binning_then_crop(hip_device, dtype, bins, width):
    """One job of mvs_register_pairs with ``bin`` set (crops from the RAW tiles, crop_bin_kernel<TIn>) against mvs_register_crops on
    crops built on the host -- numpy binning, then the same whole-pixel crop with NaN outside: equal translation, status, candidate
    count and quality (``==``).  Two raw tiles on one pixel grid, 6 x 20 x 64 binned samples each; the fixed crop is the right strip of
    its tile (every sample inside), the moving crop is shifted by (0, 1, -2) binned samples (two columns and one row outside -> NaN).
    The moving window starts one bin into its allocation along z and y (strided, non-contiguous planes).

    uint16, bins (1, 2, 2) / (3, 2, 2), even raw width (130 / 128-element rows, 4-byte aligned windows): the 8-output vector branch
    for every group that lies inside the window -- all groups of the fixed crop, width 48 (6 groups) and 51 (7 groups, the last
    moved back by 5) -- and the 4-byte pair-load branch for the moving crop's first group of each row (x - 2 < 0) and the rows outside.
    "odd_raw_width": rows of 133 elements and windows from raw x = 1 -> pairs_aligned false -> the generic branch.  bins (1, 7, 7)
    (bx != 2) and uint8 (sizeof != 2): the generic branch at every width.  With these quantised tiles the (1, 7, 7) crops hold
    constant bins whose sum * (1 / 49) truncates to one less: asserted on the host below, so the case cannot lose its point."""
    from multiview_stitcher_amd import _lib, _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    dtype = np.dtype(dtype)
    ox, odd, x0 = CROP_WIDTHS[width]
    nb = (6, 20, 64)
    raw = tuple(n * b for n, b in zip(nb, bins))
    out_shape = (nb[0], nb[1], ox)
    t_fixed, t_moving = (0, 0, nb[2] - ox), (0, 1, -2)
    # the moving tile's place in the field: where the two crops show the same scene, plus a jitter in raw pixels for the registration
    jitter = (0, 3, -2)
    origin_a = (2 * bins[0], 4 * bins[1], 4 * bins[2])
    origin_b = tuple(oa + (tf - tm) * b + j for oa, tf, tm, b, j in zip(origin_a, t_fixed, t_moving, bins, jitter))
    field = _quantised_field(tuple(max(oa, ob) + r + 2 for oa, ob, r in zip(origin_a, origin_b, raw)), (1.0, 1.5 * bins[1], 1.5 * bins[2]), dtype)
    tile_a = field[tuple(slice(o, o + r) for o, r in zip(origin_a, raw))]
    tile_b = field[tuple(slice(o, o + r) for o, r in zip(origin_b, raw))]
    row = raw[2] + x0 + 2
    row += (row % 2 == 0) if odd else (row % 2)
    assert (row % 2 == 1) == odd
    alloc_a = np.zeros((raw[0], raw[1], row), dtype)
    alloc_b = np.zeros((raw[0] + bins[0], raw[1] + bins[1], row), dtype)
    win_a = (slice(0, raw[0]), slice(0, raw[1]), slice(x0, x0 + raw[2]))
    win_b = (slice(bins[0], bins[0] + raw[0]), slice(bins[1], bins[1] + raw[1]), slice(x0, x0 + raw[2]))
    alloc_a[win_a], alloc_b[win_b] = tile_a, tile_b
    dev_a, dev_b = DeviceArray.from_host(alloc_a, 0), DeviceArray.from_host(alloc_b, 0)

    jobs = (_lib.mvs_pair_job_t * 1)()
    for view, d, t in ((jobs[0].fixed, dev_a[win_a], t_fixed), (jobs[0].moving, dev_b[win_b], t_moving)):
        assert d.shape == raw and d.strides[2] == 1
        view.data, view.dtype, view.mem = d.ptr, _lib.DTYPE_CODES[dtype], _lib.MVS_MEM_DEVICE
        view.shape[:] = list(d.shape)
        view.stride[:] = list(d.strides)
        view.matrix[:] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
        view.offset[:] = [float(v) for v in t]
        if dtype == np.uint16 and bins[2] == 2:
            aligned = d.ptr % 4 == 0 and d.strides[0] % 2 == 0 and d.strides[1] % 2 == 0
            assert aligned == (not odd)              # (pairs_aligned of crop_bin_kernel, restated on this window)
    jobs[0].out_shape[:] = list(out_shape)
    jobs[0].bin[:] = list(bins)
    t3, q = np.zeros((1, 3)), np.zeros(1)
    status, ncand, rcs = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)

    def ptr(a, ct):
        return a.ctypes.data_as(C.POINTER(ct))

    lib = _lib.init(0)
    rc = lib.mvs_register_pairs(0, 1, jobs, 3, 2, -1, 1, 1, ptr(t3, C.c_double), ptr(q, C.c_double), ptr(status, C.c_int32), ptr(ncand, C.c_int32),
                                ptr(rcs, C.c_int32))
    _lib.check(rc, 0, "mvs_register_pairs")

    crop_a = _host_crop(alloc_a[win_a], bins, t_fixed, out_shape)
    crop_b = _host_crop(alloc_b[win_b], bins, t_moving, out_shape)
    assert not np.isnan(crop_a).any() and np.isnan(crop_b[:, :, :2]).all() and np.isnan(crop_b[:, -1]).all()
    assert np.isnan(crop_b).sum() == nb[0] * (2 * nb[1] + ox - 2)
    if bins == (1, 7, 7):
        # these tiles are sensitive to the rounding of the mean: sum * (1 / count) truncates some of their bins to one less
        count = float(np.prod(bins))
        sums = _block_sums(alloc_a[win_a], bins)
        assert np.count_nonzero((sums * (1.0 / count)).astype(dtype) != _numpy_bin(alloc_a[win_a], bins)) >= 50
    # (uploaded, so that mvs_register_crops takes the steps the pair path takes after its crops: device-resident float32 crops)
    want_t, want_q, want_status, want_ncand = _reg_ops.register_crops(DeviceArray.from_host(crop_a, 0), DeviceArray.from_host(crop_b, 0), 2,
                                                                      region_mode=None, constant_check=True)
    print(f"{dtype} {bins} {width}: pairs t {t3[0]} q {q[0]!r} status {status[0]} candidates {ncand[0]}; "
          f"host crops t {want_t} q {want_q!r} status {want_status} candidates {want_ncand}")
    assert want_status == 0 and np.isfinite(want_q)
    assert int(status[0]) == want_status and int(ncand[0]) == want_ncand and int(rcs[0]) == 0
    np.testing.assert_array_equal(t3[0], want_t)
    assert q[0] == want_q
