"""GPU tests of label stitching (labels.py, csrc/mvs_labels.hip) against the numpy restatement of tests/labels_oracle.py.  Every
result is an integer, so every comparison is exact equality.

Shapes are the smallest that reach every path: rows of 131 and 70 voxels (no multiple of 64 or 4: whole 16-byte aligned chunks,
chunks off the 16-byte grid and tails), a row of 256 (every chunk whole and aligned), strided device windows, runs of one label
that cross chunks and fill whole waves, tables at half load, one entry short, and exhausted; bricks cut by the grid's edge, a
rotated view, more than 64 views on one grid."""
import ctypes as C
import functools

import numpy as np
import pytest

from multiview_stitcher_amd import _label_ops, _lib, labels
from multiview_stitcher_amd.device import is_device_array
from tests import labels_cases as lc
from tests import labels_oracle as lo

pytestmark = pytest.mark.gpu


def random_labels(shape, seed, run=(1, 3, 7), big=False, negative=False, background_rows=0, huge=False):
    """An int32 label tile of blocks of ``run`` voxels (so that rows hold runs of equal labels that are cut by the 64-voxel chunks)
    with a third of background; ``big``: ids above 65 535 among them; ``huge``: 2^31 - 1 too; ``negative``: negative ids; the first
    ``background_rows`` rows all 0 (runs that go on over whole chunks and rows)."""
    rng = np.random.default_rng(seed)
    pool = [0] * 6 + list(range(1, 13))
    if big:
        pool += [65536, 70001, 199999]
    if huge:
        pool += [2**31 - 1]
    if negative:
        pool += [-1, -7, -(2**31)]
    run = run[3 - len(shape):]
    coarse = rng.choice(np.array(pool, dtype=np.int64), [-(-n // r) for n, r in zip(shape, run)])
    tile = coarse
    for axis, r in enumerate(run):
        tile = np.repeat(tile, r, axis=axis)
    tile = np.ascontiguousarray(tile[tuple(slice(0, n) for n in shape)]).astype(np.int32)
    if background_rows:
        tile.reshape(-1, shape[-1])[:background_rows] = 0
    return tile


def given_tile(tile, source, device):
    """``tile`` as the test hands it over: the host array, a resident copy, or a strided window of a larger resident array whose rows
    start three voxels in (off the 16-byte grid)."""
    if source == "host":
        return tile
    if source == "device":
        return _label_ops.to_device(tile, device)
    big = np.full(tuple(n + p for n, p in zip(tile.shape, (2, 5, 9)[3 - tile.ndim:])), 424242, dtype=np.int32)
    window = tuple(slice(o, o + n) for o, n in zip((1, 2, 3)[3 - tile.ndim:], tile.shape))
    big[window] = tile
    dev = _label_ops.to_device(big, device)[window]
    assert not dev.is_contiguous() and dev.strides[-1] == 1
    return dev


def same_table(got, want):
    assert [a.dtype for a in got] == [np.int32, np.int32, np.uint64]
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), (got, want)


# ---- counts -------------------------------------------------------------------------------------------------------------------------
COUNT_TILES = {
    "2d_37x131": lambda: random_labels((37, 131), 1, background_rows=5),
    "3d_5x9x70": lambda: random_labels((5, 9, 70), 2),
    "2d_4x256_aligned": lambda: random_labels((4, 256), 3, run=(1, 1, 40)),
    "big_ids": lambda: random_labels((37, 131), 4, big=True),
    "negative_ids": lambda: random_labels((5, 9, 70), 5, negative=True, big=True),
    "one_label": lambda: np.full((6, 200), 3, dtype=np.int32),
}


@pytest.mark.parametrize("source", ["host", "device", "device_window"])
@pytest.mark.parametrize("name", sorted(COUNT_TILES))
def test_label_counts(name, source, hip_device):
    tile = COUNT_TILES[name]()
    want = lo.label_counts(tile)
    got = _label_ops.label_counts(given_tile(tile, source, hip_device), hip_device)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert int(got.sum()) == tile.size and got[0] >= np.count_nonzero(tile <= 0)
    if name in ("big_ids", "negative_ids"):
        assert len(want) > 65536            # the first capacity did not hold the largest label: the call was repeated


def test_label_counts_retry_with_a_small_capacity(hip_device):
    """A capacity below the largest label: the entry counts what fits, reports the largest label and is no error; the wrapper calls
    again with room for it."""
    tile = random_labels((37, 131), 1)
    want = lo.label_counts(tile)
    assert len(want) == 13
    lib = _lib.init(hip_device)
    view, keep = _label_ops.label_view(tile, None, None, hip_device)
    counts, mx = np.full(8, 99, dtype=np.uint64), C.c_int64(-1)
    _lib.check(lib.mvs_label_counts(hip_device, C.byref(view), 2, 8, counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(mx)), hip_device)
    assert mx.value == 12 and np.array_equal(counts, want[:8])
    assert np.array_equal(_label_ops.label_counts(tile, hip_device, capacity=8), want)
    assert np.array_equal(_label_ops.label_counts(tile, hip_device, capacity=13), want)       # exactly enough: one call
    sims = [lc.label_sim(tile), lc.label_sim(random_labels((5, 70), 9, big=True))]
    got = labels.label_counts(sims, device=hip_device)
    assert all(np.array_equal(g, lo.label_counts(s.data)) for g, s in zip(got, sims))


# ---- pair overlaps --------------------------------------------------------------------------------------------------------------------
def pair_case(name):
    """(sim a, sim b) on host tiles."""
    if name == "fractional_shift_2d":
        return lc.label_sim(random_labels((37, 131), 11)), lc.label_sim(random_labels((40, 90), 12, big=True, huge=True), origin=(5.5, 60.25))
    if name == "spacing_and_negative_2d":
        return (lc.label_sim(random_labels((37, 131), 13, negative=True)),
                lc.label_sim(random_labels((30, 50), 14, negative=True), origin=(-6.0, 20.0), spacing=(1.5, 2.0)))
    if name == "rotated_2d":
        return (lc.label_sim(random_labels((37, 131), 15)),
                lc.label_sim(random_labels((40, 90), 16), origin=(2.0, 40.0), affine=lc.rotation(2, 17.0, (20.0, 80.0), (1.25, -3.5))))
    if name == "rotated_3d":
        return (lc.label_sim(random_labels((5, 9, 70), 17)),
                lc.label_sim(random_labels((6, 12, 40), 18), origin=(-1.0, -2.0, 20.0), affine=lc.rotation(3, -11.0, (2.0, 4.0, 40.0), (0.5, 0.0, 0.75))))
    if name == "one_label_each":      # whole-wave runs, carried from chunk to chunk
        return lc.label_sim(np.full((40, 200), 7, dtype=np.int32)), lc.label_sim(np.full((40, 200), 9, dtype=np.int32), origin=(3.0, 10.0))
    if name == "arange_64x64":        # every voxel a distinct pair
        a = np.arange(1, 4097, dtype=np.int32).reshape(64, 64)
        return lc.label_sim(a), lc.label_sim(a.copy(), origin=(1.0, 0.0))
    raise KeyError(name)


PAIR_CASES = ["fractional_shift_2d", "spacing_and_negative_2d", "rotated_2d", "rotated_3d", "one_label_each", "arange_64x64"]


@functools.lru_cache(maxsize=None)
def pair_want(name):
    return lc.oracle_pair_table(*pair_case(name))


def as_given(sim_pair, source, device):
    a, b = sim_pair
    return [a.copy(data=given_tile(a.data, source, device)), b.copy(data=given_tile(b.data, "host" if source == "host" else "device", device))]


@pytest.mark.parametrize("source", ["host", "device_window"])
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pair_overlaps(name, source, hip_device):
    want = pair_want(name)
    assert len(want[0]) > 0
    got = labels.pair_overlaps(as_given(pair_case(name), source, hip_device), lc.KEY, pairs=[(0, 1)], device=hip_device)
    assert list(got) == [(0, 1)]
    same_table(got[(0, 1)], want)
    if name == "one_label_each":
        assert want[0].tolist() == [7] and want[1].tolist() == [9] and want[2].tolist() == [37 * 190]
    if name == "arange_64x64":
        assert len(want[0]) == 63 * 64 and (want[2] == 1).all()


def test_pair_overlaps_default_pairs_and_no_overlap(hip_device):
    """The default pairs are the edges of the overlap graph; a pair that is asked for and does not overlap has an empty table."""
    a, b = pair_case("fractional_shift_2d")
    far = lc.label_sim(random_labels((20, 30), 19), origin=(500.0, 0.0))
    got = labels.pair_overlaps([a, b, far], lc.KEY, device=hip_device)
    assert list(got) == [(0, 1)]
    same_table(got[(0, 1)], pair_want("fractional_shift_2d"))
    got = labels.pair_overlaps([a, b, far], lc.KEY, pairs=[(2, 0)], device=hip_device)
    assert list(got) == [(0, 2)] and all(len(x) == 0 for x in got[(0, 2)])
    # a box that is not empty in which b is nowhere in bounds: the kernel's own test
    matrix, offset = lc.pair_affine(a, far)
    same_table(_label_ops.pair_overlaps(a.data, far.data, matrix, offset, [0, 0], [37, 131], hip_device), lo.pair_table(a.data, far.data, matrix, offset))


def raw_pair_call(a, b, capacity, device):
    """mvs_label_pair_overlaps itself over the whole of tile a: (return code, n_unique, the triples it wrote, sorted)."""
    lib = _lib.init(device)
    matrix, offset = lc.pair_affine(a, b)
    va, ka = _label_ops.label_view(a.data, None, None, device)
    vb, kb = _label_ops.label_view(b.data, matrix, offset, device)
    la, lb, n = np.zeros(capacity, np.int32), np.zeros(capacity, np.int32), np.zeros(capacity, np.uint64)
    nu = C.c_int64(-1)
    ndim = a.data.ndim
    rc = lib.mvs_label_pair_overlaps(device, C.byref(va), C.byref(vb), ndim, _lib.i64x3([0, 0, 0]), _lib.i64x3([1] * (3 - ndim) + list(a.data.shape)),
                                     capacity, la.ctypes.data_as(C.POINTER(C.c_int32)), lb.ctypes.data_as(C.POINTER(C.c_int32)),
                                     n.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(nu))
    k = min(int(nu.value), capacity)
    order = np.lexsort((lb[:k], la[:k]))
    return rc, int(nu.value), (la[:k][order], lb[:k][order], n[:k][order])


def test_pair_table_at_its_designed_load(hip_device):
    """4032 distinct pairs with a capacity of 4096: 8192 slots, half full.  The whole table comes back from one call."""
    a, b = pair_case("arange_64x64")
    rc, n_unique, got = raw_pair_call(a, b, 4096, hip_device)
    assert rc == 0 and n_unique == 63 * 64
    same_table(got, pair_want("arange_64x64"))
    matrix, offset, box_lo, box_n = labels.pair_geometry(a, b, lc.KEY)
    same_table(_label_ops.pair_overlaps(a.data, b.data, matrix, offset, box_lo, box_n, hip_device, capacity=4096), pair_want("arange_64x64"))


def test_pair_capacity_one_below_n_unique(hip_device):
    """One entry short: the call reports n_unique and MVS_LABEL_INCOMPLETE, which is no error, writes `capacity` entries of the table
    -- each with its right count -- and the wrapper succeeds on its second call."""
    a, b = pair_case("fractional_shift_2d")
    want = pair_want("fractional_shift_2d")
    n_true = len(want[0])
    rc, n_unique, got = raw_pair_call(a, b, n_true - 1, hip_device)
    assert rc == _lib.MVS_LABEL_INCOMPLETE and n_unique == n_true
    table = {(x, y): z for x, y, z in zip(*[w.tolist() for w in want])}
    assert len(got[0]) == n_true - 1 and len(set(zip(got[0].tolist(), got[1].tolist()))) == n_true - 1
    assert all(table[(x, y)] == z for x, y, z in zip(*[g.tolist() for g in got]))
    rc, n_unique, got = raw_pair_call(a, b, n_true, hip_device)          # exactly enough
    assert rc == 0 and n_unique == n_true
    same_table(got, want)
    matrix, offset, box_lo, box_n = labels.pair_geometry(a, b, lc.KEY)
    same_table(_label_ops.pair_overlaps(a.data, b.data, matrix, offset, box_lo, box_n, hip_device, capacity=n_true - 1), want)


def test_pair_table_exhausted_is_reported_not_waited_for(hip_device):
    """4032 distinct pairs into the 1024 slots behind a capacity of 16: probing is bounded by the table, the voxels that find no slot
    are dropped, the call comes back with MVS_LABEL_INCOMPLETE and the number of slots, and the wrapper grows until the table is
    whole."""
    a, b = pair_case("arange_64x64")
    rc, n_unique, got = raw_pair_call(a, b, 16, hip_device)
    assert rc == _lib.MVS_LABEL_INCOMPLETE and n_unique == 1024 and len(got[0]) == 16
    matrix, offset, box_lo, box_n = labels.pair_geometry(a, b, lc.KEY)
    same_table(_label_ops.pair_overlaps(a.data, b.data, matrix, offset, box_lo, box_n, hip_device, capacity=16), pair_want("arange_64x64"))


# ---- fuse ---------------------------------------------------------------------------------------------------------------------------
def random_luts(sims, seed, short=None):
    """Per view a table over its labels with random ids (lut[0] == 0); ``short``: the view whose table ends below its largest label."""
    rng = np.random.default_rng(seed)
    luts = []
    for v, s in enumerate(sims):
        lut = rng.integers(1, 5000, int(np.asarray(s.data).max()) + 1).astype(np.int32)
        lut[0] = 0
        luts.append(lut[:7] if v == short else lut)
    return luts


def fuse_case(name):
    """(sims on host tiles, luts)"""
    if name == "three_2d_one_rotated":
        sims = [lc.label_sim(random_labels((37, 131), 21)), lc.label_sim(random_labels((40, 90), 22), origin=(20.5, 100.25)),
                lc.label_sim(random_labels((50, 60), 23), origin=(10.0, 50.0), affine=lc.rotation(2, 23.0, (35.0, 80.0), (0.5, 2.0)))]
        return sims, random_luts(sims, 1)
    if name == "two_3d":
        sims = [lc.label_sim(random_labels((5, 9, 70), 24)), lc.label_sim(random_labels((6, 11, 40), 25), origin=(1.5, 3.0, 50.25))]
        return sims, random_luts(sims, 2)
    if name == "identical_geometry_tie":
        sims = [lc.label_sim(random_labels((20, 70), 26)), lc.label_sim(random_labels((20, 70), 27) + 20)]
        return sims, random_luts(sims, 3)
    if name == "short_lut":
        sims = [lc.label_sim(random_labels((20, 70), 28)), lc.label_sim(random_labels((24, 66), 29), origin=(4.0, 30.0))]
        return sims, random_luts(sims, 4, short=1)
    if name == "identity_negative_big":
        sims = [lc.label_sim(random_labels((20, 70), 30, negative=True, big=True, huge=True)),
                lc.label_sim(random_labels((24, 66), 31, negative=True), origin=(4.0, 30.5))]
        return sims, None
    if name == "mixed_identity":
        sims, luts = fuse_case("short_lut")
        return sims, [None, luts[1]]
    if name == "seventy_views":       # one row of 70 small tiles, each over half of the next: culling goes past 64 views
        sims = [lc.label_sim(random_labels((8, 20), 100 + v) + 13 * v, origin=(float(v % 3), 9.0 * v)) for v in range(70)]
        return sims, random_luts(sims, 5)
    raise KeyError(name)


FUSE_CASES = ["three_2d_one_rotated", "two_3d", "identical_geometry_tie", "short_lut", "identity_negative_big", "mixed_identity", "seventy_views"]


@functools.lru_cache(maxsize=None)
def fuse_want(name):
    sims, luts = fuse_case(name)
    return lc.oracle_fuse(sims, luts)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", FUSE_CASES)
def test_fuse_label_tiles(name, where, hip_device):
    sims, luts = fuse_case(name)
    want = fuse_want(name)
    if where == "device":
        sims = [s.copy(data=given_tile(s.data, "device_window" if v % 2 else "device", hip_device)) for v, s in enumerate(sims)]
    res = labels.fuse_label_tiles(sims, lc.KEY, luts=luts, device=hip_device, output_on_backend=where == "device")
    assert is_device_array(res.data) == (where == "device")
    got = res.data.get() if where == "device" else res.data
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    if name == "identical_geometry_tie":
        assert np.array_equal(want, luts[0][fuse_case(name)[0][0].data])      # view 0 everywhere
    if name == "short_lut":
        assert np.asarray(fuse_case(name)[0][1].data).max() >= 7 and (want == 0).any()
    if name == "seventy_views":
        assert want.shape[1] > 64 * 9 and len(sims) == 70


@pytest.mark.parametrize("name", ["three_2d_one_rotated", "two_3d"])
def test_fuse_box_equals_the_crop_of_the_whole(name, hip_device):
    """A box of the whole grid -- first voxel off the brick grid, last bricks cut -- equals the crop of the whole result, and a box
    that reaches beyond the grid is 0 there."""
    sims, luts = fuse_case(name)
    want = fuse_want(name)
    grid = lc.whole_grid(sims)
    first, shape = ((5, 17), (21, 83)) if want.ndim == 2 else ((1, 2, 9), (3, 5, 70))
    crop = tuple(slice(f, f + n) for f, n in zip(first, shape))
    part = labels.fuse_label_tiles(sims, lc.KEY, luts=luts, output_stack_properties=lc.sub_grid(grid, first, shape), device=hip_device)
    assert np.array_equal(part.data, want[crop])
    assert np.array_equal(part.data, lc.oracle_fuse(sims, luts, box=(list(first), list(shape))))
    first = tuple(-3 for _ in first)
    shape = tuple(n + 6 for n in want.shape)
    padded = labels.fuse_label_tiles(sims, lc.KEY, luts=luts, output_stack_properties=lc.sub_grid(grid, first, shape), device=hip_device)
    inner = tuple(slice(3, 3 + n) for n in want.shape)
    assert np.array_equal(padded.data[inner], want)
    outside = np.ones(shape, dtype=bool)
    outside[inner] = False
    assert (padded.data[outside] == 0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["host", "device"])
def test_stitch_labels_disc_mosaic(source, hip_device):
    """82 discs cut into 2 x 2 overlapping tiles at integer offsets, every tile relabelled at random with ids up to 199 999: the
    stitched image is the truth up to a bijection, with 82 objects, and equals the oracle's run voxel for voxel."""
    truth, tiles, sims = lc.disc_mosaic()
    given = [s.copy(data=given_tile(s.data, source, hip_device)) for s in sims]
    res = labels.stitch_labels(given, lc.KEY, device=hip_device)
    assert res.attrs["n_objects"] == lc.N_DISCS
    assert res.data.shape == truth.shape and lo.same_up_to_bijection(res.data, truth)
    cnt = [lo.label_counts(t) for t in tiles]
    ov = {(a, b): lc.oracle_pair_table(sims[a], sims[b]) for a, b in labels.view_pairs(sims, lc.KEY)}
    luts, n = lo.match_labels(cnt, ov)
    assert n == lc.N_DISCS and np.array_equal(res.data, lc.oracle_fuse(sims, luts))
    # what the matching is for: painted without it, an object that lies in two tiles keeps two ids
    assert not lo.same_up_to_bijection(labels.fuse_label_tiles(given, lc.KEY, device=hip_device).data, truth)
