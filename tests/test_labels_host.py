"""CPU: the host side of label stitching (labels.py): the matching of labels into objects, the geometry the drivers hand to the
kernels (under a recording stand-in for ``_label_ops``), the conversions and refusals that need no device, the refusals of the C
entries before any device is touched, csrc/mvs_labels_plan.h compiled for the host under the address and undefined-behaviour
sanitizers, and the disc mosaic end to end through the oracle alone (tests/labels_oracle.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from multiview_stitcher_amd import _label_ops, _lib, labels, msi_utils
from multiview_stitcher_amd import spatial_image_utils as si
from tests import labels_cases as lc
from tests import labels_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def table(rows):
    """(la, lb, n) arrays of a list of rows."""
    rows = sorted(rows)
    return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.uint64))


def counts(*per_view):
    """Per view {label: count} as count arrays."""
    out = []
    for c in per_view:
        a = np.zeros(max(c) + 1, dtype=np.uint64)
        for label, n in c.items():
            a[label] = n
        out.append(a)
    return out


# ---- match_labels -------------------------------------------------------------------------------------------------------------------
def test_match_numbering_follows_the_smallest_member():
    """Objects are numbered by their smallest (view, label): view 0's labels first, in label order, whatever they merge with."""
    cnt = counts({0: 50, 2: 10, 5: 10, 7: 10}, {0: 60, 1: 10, 3: 10, 9: 10})
    ov = {(0, 1): table([(5, 1, 10), (2, 9, 10), (0, 3, 4), (7, 0, 3)])}
    luts, n = labels.match_labels(cnt, ov)
    assert n == 4
    assert luts[0].tolist() == [0, 0, 1, 0, 0, 2, 0, 3]          # labels 2, 5, 7 -> 1, 2, 3; labels without a voxel -> 0
    assert luts[1].tolist() == [0, 2, 0, 4, 0, 0, 0, 0, 0, 1]    # 1 joins (0, 5), 9 joins (0, 2), 3 is an object of its own
    assert all(l.dtype == np.int32 and l[0] == 0 for l in luts)
    want, want_n = lo.match_labels(cnt, ov)
    assert want_n == n and all(np.array_equal(a, b) for a, b in zip(luts, want))


@pytest.mark.parametrize("criterion", ["iou", "min_fraction"])
def test_match_threshold_is_inclusive(criterion):
    """A score of exactly the threshold joins; the next float below does not.  iou: 1 / (2 + 1 - 1) = 0.5; min_fraction: 1 / min(2,
    4) = 0.5 (the zero rows carry the marginals)."""
    cnt = counts({0: 10, 1: 2}, {0: 10, 1: 4})
    rows = [(1, 1, 1), (1, 0, 1)] if criterion == "iou" else [(1, 1, 1), (1, 0, 1), (0, 1, 3)]
    ov = {(0, 1): table(rows)}
    luts, n = labels.match_labels(cnt, ov, criterion=criterion, threshold=0.5)
    assert n == 1 and luts[0][1] == luts[1][1] == 1
    luts, n = labels.match_labels(cnt, ov, criterion=criterion, threshold=np.nextafter(0.5, 1.0))
    assert n == 2 and (luts[0][1], luts[1][1]) == (1, 2)
    for thr in (0.5, np.nextafter(0.5, 1.0)):
        want, want_n = lo.match_labels(cnt, ov, criterion, thr)
        got, got_n = labels.match_labels(cnt, ov, criterion=criterion, threshold=thr)
        assert want_n == got_n and all(np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(ValueError):
        labels.match_labels(cnt, ov, criterion="dice")


def test_match_min_voxels():
    cnt = counts({0: 10, 1: 3}, {0: 10, 1: 3})
    ov = {(0, 1): table([(1, 1, 3)])}
    assert labels.match_labels(cnt, ov, min_voxels=3)[1] == 1      # n >= min_voxels
    assert labels.match_labels(cnt, ov, min_voxels=4)[1] == 2
    assert lo.match_labels(cnt, ov, min_voxels=4)[1] == 2


def test_match_chain_merges_transitively_and_lonely_labels_get_ids():
    """a-b and b-c make one object of three labels that never meet in one table; labels absent from every overlap are objects."""
    cnt = counts({0: 5, 1: 9, 2: 9}, {0: 5, 4: 9}, {0: 5, 2: 9, 6: 1})
    ov = {(0, 1): table([(2, 4, 6)]), (1, 2): table([(4, 2, 6)]), (0, 2): table([])}
    luts, n = labels.match_labels(cnt, ov)
    assert n == 3
    assert luts[0].tolist() == [0, 1, 2] and luts[1].tolist() == [0, 0, 0, 0, 2] and luts[2].tolist() == [0, 0, 2, 0, 0, 0, 3]
    want, want_n = lo.match_labels(cnt, ov)
    assert want_n == 3 and all(np.array_equal(a, b) for a, b in zip(luts, want))
    # no overlaps at all: every label its own object, numbered view by view
    luts, n = labels.match_labels(cnt, {})
    assert n == 5 and luts[2].tolist() == [0, 0, 4, 0, 0, 0, 5]
    with pytest.raises(ValueError):                                  # an edge to a label that has no voxel
        labels.match_labels(cnt, {(0, 1): table([(2, 3, 6)])})


def test_match_random_tables_equal_the_oracle():
    rng = np.random.default_rng(17)
    for criterion in ("iou", "min_fraction"):
        cnt = [np.r_[100, rng.integers(0, 3, 30) * 20].astype(np.uint64) for _ in range(4)]
        ov = {}
        for a, b in [(0, 1), (1, 2), (2, 3), (0, 3)]:
            la_ok, lb_ok = np.nonzero(cnt[a])[0], np.nonzero(cnt[b])[0]
            rows = {(int(rng.choice(la_ok)), int(rng.choice(lb_ok))): int(rng.integers(1, 12)) for _ in range(40)}
            rows.pop((0, 0), None)
            ov[(a, b)] = table([(x, y, n) for (x, y), n in rows.items()])
        got, got_n = labels.match_labels(cnt, ov, criterion=criterion, threshold=0.3, min_voxels=2)
        want, want_n = lo.match_labels(cnt, ov, criterion, 0.3, 2)
        assert got_n == want_n and 1 < got_n < sum(int(np.count_nonzero(c[1:])) for c in cnt)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- the drivers under a recording stand-in -------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for ``_label_ops``: records what the drivers hand to the array level and answers through the oracle."""

    def __init__(self):
        self.calls = []

    def label_counts(self, tile, device=0, capacity=None):
        self.calls.append(("counts", tile, device))
        return lo.label_counts(tile)

    def pair_overlaps(self, a, b, matrix, offset, box_lo, box_n, device=0, capacity=None):
        self.calls.append(("pairs", a, b, matrix, offset, box_lo, box_n, device))
        return lo.pair_table(a, b, matrix, offset)

    def fuse_label_tiles(self, tiles, matrices, offsets, luts, out_shape, index_origin=None, device=0, out_on_device=False):
        self.calls.append(("fuse", tiles, matrices, offsets, luts, out_shape, index_origin, device, out_on_device))
        return lo.fuse(tiles, matrices, offsets, luts, tuple(out_shape), index_origin)


@pytest.fixture
def recorder(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(labels, "_label_ops", r)
    return r


def test_pair_overlaps_driver_hands_over_affine_and_box(recorder):
    rng = np.random.default_rng(2)
    tiles = [rng.integers(0, 4, (20, 30)).astype(np.int32) for _ in range(3)]
    sims = [lc.label_sim(tiles[0]), lc.label_sim(tiles[1], origin=(4.5, 22.0)), lc.label_sim(tiles[2], origin=(100.0, 0.0))]
    got = labels.pair_overlaps(sims, lc.KEY, device=3)
    assert list(got) == [(0, 1)]                                   # the edges of the overlap graph: view 2 is far away
    (_, a, b, matrix, offset, box_lo, box_n, device), = recorder.calls
    assert a is tiles[0] and b is tiles[1] and device == 3
    want_m, want_o = lc.pair_affine(sims[0], sims[1])
    assert np.array_equal(matrix, want_m) and np.array_equal(offset, want_o) and offset.tolist() == [-4.5, -22.0]
    # b covers rows 4.5 .. 23.5 and columns 22 .. 51 of a: the box bounds that, with a margin, inside a
    lo_, hi_ = np.array(box_lo), np.array(box_lo) + np.array(box_n) - 1
    assert lo_[0] <= 4 and lo_[1] <= 22 and hi_.tolist() == [19, 29] and (lo_ >= 0).all()
    assert all(np.array_equal(x, y) for x, y in zip(got[(0, 1)], lc.oracle_pair_table(sims[0], sims[1])))
    # given pairs: used once each, the lower index as a; a far pair gets an empty box
    recorder.calls.clear()
    labels.pair_overlaps(sims, lc.KEY, pairs=[(1, 0), (0, 1), (2, 0)])
    assert [(c[1] is tiles[0], c[2] is tiles[1] or c[2] is tiles[2]) for c in recorder.calls] == [(True, True)] * 2
    assert min(recorder.calls[1][6]) == 0
    with pytest.raises(ValueError):
        labels.pair_overlaps(sims, lc.KEY, pairs=[(1, 1)])


def test_footprint_box_of_a_rotated_tile_bounds_every_in_bounds_voxel():
    a, b = lc.label_sim(np.zeros((40, 50), np.int32)), lc.label_sim(np.zeros((30, 20), np.int32), origin=(5.0, 25.0),
                                                                   affine=lc.rotation(2, 25.0, (20.0, 30.0)))
    matrix, offset, box_lo, box_n = labels.pair_geometry(a, b, lc.KEY)
    inside = lo.in_bounds(lo.coordinates(matrix, offset, (40, 50)), (30, 20))
    ys, xs = np.nonzero(inside)
    assert inside.any() and not inside.all()
    assert box_lo[0] <= ys.min() and box_lo[1] <= xs.min() and box_lo[0] + box_n[0] > ys.max() and box_lo[1] + box_n[1] > xs.max()
    assert box_n[0] * box_n[1] < 40 * 50
    assert labels.footprint_box(np.zeros((2, 2)), np.zeros(2), (40, 50), (30, 20)) == ([0, 0], [40, 50])      # singular: the whole tile


def test_fuse_driver_frames_and_boxes(recorder):
    rng = np.random.default_rng(4)
    tiles = [rng.integers(-1, 6, (24, 40)).astype(np.int32) for _ in range(2)]
    sims = [lc.label_sim(tiles[0]), lc.label_sim(tiles[1], origin=(3.0, 30.5))]
    grid = lc.whole_grid(sims)
    res = labels.fuse_label_tiles(sims, lc.KEY, device=2)
    _, given, matrices, offsets, luts, out_shape, origin, device, on_dev = recorder.calls[-1]
    assert given[0] is tiles[0] and luts is None and device == 2 and not on_dev
    assert list(out_shape) == [grid["shape"]["y"], grid["shape"]["x"]] and list(origin) == [0, 0]
    assert res.data.dtype == np.int32 and np.array_equal(res.data, lc.oracle_fuse(sims))
    assert si.get_origin_from_sim(res) == grid["origin"] and np.array_equal(si.get_affine_from_sim(res, lc.KEY), np.eye(3))
    # a box of the whole grid: the same view parameters, an integer index origin, and the crop of the whole result
    box = lc.sub_grid(grid, (5, 17), (11, 23))
    part = labels.fuse_label_tiles(sims, lc.KEY, output_stack_properties=box)
    call = recorder.calls[-1]
    assert all(np.array_equal(x, y) for x, y in zip(call[2], matrices)) and all(np.array_equal(x, y) for x, y in zip(call[3], offsets))
    assert list(call[6]) == [5, 17] and list(call[5]) == [11, 23]
    assert np.array_equal(part.data, res.data[5:16, 17:40]) and si.get_origin_from_sim(part) == box["origin"]
    # a grid that is no box of it (half a voxel off): a frame of its own, index origin zero
    off = lc.sub_grid(grid, (5.5, 17), (11, 23))
    labels.fuse_label_tiles(sims, lc.KEY, output_stack_properties=off)
    call = recorder.calls[-1]
    assert list(call[6]) == [0, 0] and not np.array_equal(call[3][0], offsets[0])


def test_stitch_driver_runs_the_four_in_sequence(recorder):
    truth, tiles, sims = lc.disc_mosaic()
    res = labels.stitch_labels([msi_utils.get_msim_from_sim(s) for s in sims[:2]] + sims[2:], lc.KEY, device=1)
    kinds = [c[0] for c in recorder.calls]
    assert kinds == ["counts"] * 4 + ["pairs"] * 6 + ["fuse"]
    assert all(c[-1] == 1 for c in recorder.calls if c[0] != "fuse") and recorder.calls[-1][7] == 1
    assert res.attrs["n_objects"] == lc.N_DISCS and lo.same_up_to_bijection(res.data, truth)


def test_conversions_and_refusals_need_no_device():
    assert _label_ops.as_label_tile(np.array([[1, 70000]], np.uint32)).dtype == np.int32
    assert _label_ops.as_label_tile(np.array([[3, -(2**40)]], np.int64)).tolist() == [[3, -1]]      # negative: background, whatever its size
    with pytest.raises(ValueError, match="2\\^31"):
        _label_ops.as_label_tile(np.array([[1, 2**31]], np.int64))
    with pytest.raises(ValueError, match="2\\^31"):
        _label_ops.as_label_tile(np.array([[2**32 - 1]], np.uint32))
    with pytest.raises(TypeError):
        _label_ops.as_label_tile(np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        _label_ops.as_label_tile(np.zeros(3, np.int32))
    tile = np.zeros((4, 5), np.int32)
    t_sim = si.to_spatial_image(np.zeros((2, 4, 5), np.int32), dims=["t", "y", "x"], scale={"y": 1.0, "x": 1.0}, translation={"y": 0.0, "x": 0.0})
    for call in (lambda s: labels.label_counts(s), lambda s: labels.pair_overlaps(s, lc.KEY), lambda s: labels.fuse_label_tiles(s, lc.KEY),
                 lambda s: labels.stitch_labels(s, lc.KEY)):
        with pytest.raises(NotImplementedError, match="label_sims\\[1\\]"):
            call([lc.label_sim(tile), t_sim])
        with pytest.raises(ValueError):
            call([])


def test_entries_refuse_bad_arguments_before_any_device():
    """The checks that come before mvs_check_ready: codes, never a crash, on a machine without a GPU too."""
    lib = _lib.load()
    tile = np.zeros((4, 6), np.int32)
    view, keep = _label_ops.label_view(tile, None, None, 0)
    cnt, mx = np.zeros(4, np.uint64), C.c_int64()
    u64, i32, i64 = C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    assert lib.mvs_label_counts(0, C.byref(view), 2, 0, cnt.ctypes.data_as(u64), C.byref(mx)) == -1
    assert lib.mvs_label_counts(0, C.byref(view), 2, (1 << 31) + 1, cnt.ctypes.data_as(u64), C.byref(mx)) == _lib.ERR_UNSUPPORTED
    assert lib.mvs_label_counts(0, C.byref(view), 4, 4, cnt.ctypes.data_as(u64), C.byref(mx)) == -1
    assert lib.mvs_label_counts(0, None, 2, 4, cnt.ctypes.data_as(u64), C.byref(mx)) == -1
    strided = _lib.mvs_view_t.from_buffer_copy(view)
    strided.stride[2] = 2
    assert lib.mvs_label_counts(0, C.byref(strided), 2, 4, cnt.ctypes.data_as(u64), C.byref(mx)) == _lib.ERR_UNSUPPORTED
    la, lb, n, nu = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint64), C.c_int64()
    pair = lambda lo3, n3, cap: lib.mvs_label_pair_overlaps(0, C.byref(view), C.byref(view), 2, _lib.i64x3(lo3), _lib.i64x3(n3), cap,
                                                           la.ctypes.data_as(i32), lb.ctypes.data_as(i32), n.ctypes.data_as(u64), C.byref(nu))
    assert pair([0, 0, 0], [1, 4, 7], 4) == -1          # the box leaves the tile
    assert pair([0, 0, 0], [1, 0, 6], 4) == -1          # an empty box
    assert pair([0, 0, 0], [1, 4, 6], 0) == -1
    assert pair([0, 0, 0], [1, 4, 6], (1 << 27) + 1) == _lib.ERR_UNSUPPORTED
    out = np.zeros((4, 6), np.int32)
    fuse = lambda shape, origin: lib.mvs_label_tiles_fuse(0, C.byref(view), 1, 2, None, None, _lib.i64x3(shape), _lib.i64x3(origin),
                                                          C.c_void_p(out.ctypes.data), _lib.MVS_MEM_HOST)
    assert fuse([2, 4, 6], [0, 0, 0]) == -1             # a 2D grid with two planes
    assert fuse([1, 0, 6], [0, 0, 0]) == -1
    assert fuse([1, 4, 6], [0, 0, 2**31 - 3]) == -1     # the box leaves the int32 index range
    del keep


def test_plan_header_under_sanitizers(tmp_path):
    """tests/native/labels_plan_host_test.cpp: a stand-alone program of mvs_labels_plan.h -- the table's size, the probe sequence that
    visits every slot once, the bounded insertion filled to the last slot and one beyond, the launch geometry -- built with the host
    compiler and -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "labels_plan_host_test"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "labels_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    slots = {int(ln.split()[1]): int(ln.split()[2]) for ln in lines if ln.startswith("S ")}
    assert slots == {0: 0, 1: 1024, 512: 1024, 513: 2048, 4096: 8192, 65536: 131072, (1 << 27): 1 << 28, (1 << 27) + 1: 0}
    fill = {ln.split()[1]: [int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("F ")}
    assert fill["seam"] == [4096, 4096, 0]              # 4096 neighbouring pairs into 8192 slots: all found again, none dropped
    assert fill["full"] == [1024, 1024, 0]              # as many keys as slots: the last one still finds the last free slot
    assert fill["beyond"] == [1030, 1024, 6]            # six more: dropped after exactly `slots` probes each
    waves = {tuple(int(v) for v in ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in lines if ln.startswith("W ")}
    assert waves[(10, 4)] == [3, 1] and waves[(8192, 8192)] == [1, 1] and waves[(8193, 8192)] == [2, 1] and waves[(0, 4)] == [0, 1]


# ---- end to end through the oracle alone -------------------------------------------------------------------------------------------
def test_disc_mosaic_through_the_oracle():
    """82 discs on 96 x 150, cut into 2 x 2 tiles of 56 x 85 with random ids per tile: counts, tables, matching and fusion of the
    oracle give the truth back up to a bijection, with 82 objects."""
    truth, tiles, sims = lc.disc_mosaic()
    assert truth.shape == (96, 150) and len(np.unique(truth)) == lc.N_DISCS + 1 and all(t.shape == (56, 85) for t in tiles)
    assert max(int(t.max()) for t in tiles) > 65535
    cnt = [lo.label_counts(t) for t in tiles]
    pairs = labels.view_pairs(sims, lc.KEY)
    assert pairs == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    ov = {(a, b): lc.oracle_pair_table(sims[a], sims[b]) for a, b in pairs}
    assert all(len(t[0]) > 0 for t in ov.values())                 # every overlap, the diagonal ones included, holds a disc
    luts, n = lo.match_labels(cnt, ov)
    assert n == lc.N_DISCS
    fused = lc.oracle_fuse(sims, luts)
    assert fused.shape == truth.shape and lo.same_up_to_bijection(fused, truth) and fused.max() == lc.N_DISCS
    # without the matching an object that lies in two tiles keeps two ids
    assert not lo.same_up_to_bijection(lc.oracle_fuse(sims, None), truth)
