"""CPU: connected-component labelling (labels.label_components, csrc/mvs_components.hip) without a device: the test masks have the
properties their names claim (through the oracle alone, tests/components_oracle.py), the refusals of the Python layers and of the C
entry before any device is touched, the driver under a recording stand-in for ``_label_ops``, the disc mosaic end to end through the
oracles alone, and tests/native/components_host_test.cpp -- csrc/mvs_components_plan.h and the shared union / find of
csrc/mvs_unionfind.h on CPU threads -- built with the host compiler under the sanitizers and run directly."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from multiview_stitcher_amd import _label_ops, _lib, labels, msi_utils
from multiview_stitcher_amd import spatial_image_utils as si
from tests import components_cases as cc
from tests import components_oracle as co
from tests import labels_cases as lc
from tests import labels_oracle as lo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the cases through the oracle alone ---------------------------------------------------------------------------------------------
def test_oracle_rules():
    tile = np.array([[0.5, np.nan, 0.50000006, -np.inf, np.inf, 0.4]], np.float32)
    assert co.foreground(tile, 0.5).tolist() == [[False, False, True, False, True, False]]
    assert co.foreground(np.array([[0, 1, 255]], np.uint8), 0).tolist() == [[False, True, True]]
    assert co.foreground(np.array([[300, 301]], np.uint16), 300.0000001).tolist() == [[False, True]]      # the threshold is rounded to float32
    m = np.array([[1, 0, 1, 1, 0, 1, 1, 1]], bool)
    assert co.label_mask(m)[0].tolist() == [[1, 0, 2, 2, 0, 3, 3, 3]]
    assert co.label_mask(m, 1, 2)[0].tolist() == [[0, 0, 1, 1, 0, 2, 2, 2]] and co.label_mask(m, 1, 2)[1] == 2
    assert co.label_mask(m, 1, 3)[0].tolist() == [[0, 0, 0, 0, 0, 1, 1, 1]] and co.label_mask(m, 1, 4)[1] == 0
    d = np.array([[1, 0], [0, 1]], bool)
    assert co.label_mask(d, 1)[1] == 2 and co.label_mask(d, 2)[1] == 1


def test_cases_have_the_properties_claimed():
    n = lambda name, conn: cc.want(name, conn)[1]
    assert n("serpentine", 1) == 1 and cc.mask("serpentine").sum() == 19 * 131 + 18
    assert n("comb", 1) == 1 and co.label_mask(cc.mask("comb")[:-1], 1)[1] == 66          # without the last row: 66 teeth
    labels_u, n_u = cc.want("nested_u", 1)
    assert n_u == 3 and labels_u[0, 40] == 1 and labels_u[3, 0] == 1 and labels_u[1, 10] == 2 and labels_u[2, 30] == 2 and labels_u[5, 20] == 3
    assert n("checkerboard", 1) == int(cc.mask("checkerboard").sum()) == 2424 and n("checkerboard", 2) == 1
    assert n("all_foreground", 1) == n("all_foreground", 2) == 1 and n("all_background", 1) == 0
    assert n("single_voxel", 1) == 1 and cc.mask("single_voxel").shape == (1, 1)
    assert n("row_300", 1) == 4 and cc.mask("row_300").shape == (1, 300)
    assert cc.mask("volume_5x1x9").shape == (5, 1, 9) and n("volume_5x1x9", 1) > n("volume_5x1x9", 2) >= n("volume_5x1x9", 3) >= 1
    for name in ("random_2d_10", "random_2d_50", "random_2d_90", "random_3d_10", "random_3d_50", "random_3d_90"):
        counts = [n(name, conn) for conn in cc.connectivities(name)]
        assert counts == sorted(counts, reverse=True) and counts[-1] >= 1, (name, counts)
        assert counts[0] > counts[-1] or name.endswith("_90"), (name, counts)      # (at 90 % the 3-D mask is one component already)
    # more than 8192 chunks of 64 voxels: the waves of the row launches take two chunks each
    for name in cc.WIDE:
        shape = cc.mask(name).shape
        assert int(np.prod(shape[:-1])) * -(-shape[-1] // 64) > 8192
    runs = cc.mask("runs_across_ranges")
    assert n("runs_across_ranges", 1) == n("runs_across_ranges", 2) == int((np.diff(np.pad(runs, ((0, 0), (1, 0))).astype(np.int8), axis=1) == 1).sum())
    assert runs[0].all() and n("all_foreground_wide", 1) == 1
    assert n("volume_40x70x131", 1) > 2048 > 0 and cc.want("volume_40x70x131", 1)[0].max() == n("volume_40x70x131", 1)
    # min_voxels: some components go, some stay, and the ids stay in order
    full, n_full = cc.want("random_2d_50", 1)
    part, n_part = cc.want("random_2d_50", 1, 5)
    assert 0 < n_part < n_full and np.array_equal(part > 0, np.isin(full, np.nonzero(np.bincount(full.ravel())[1:] >= 5)[0] + 1))
    first = [int(np.flatnonzero(part.ravel() == k)[0]) for k in range(1, n_part + 1)]
    assert first == sorted(first)
    t = cc.float_tile()
    fg = co.foreground(t, cc.FLOAT_THRESHOLD)
    assert np.isnan(t).sum() > 100 and (t == np.float32(0.5)).sum() > 100 and not fg[np.isnan(t)].any() and not fg[t == np.float32(0.5)].any()
    assert fg[4, 60:70].all() and fg[np.isposinf(t)].all() and not fg[np.isneginf(t)].any()
    for dtype in (np.uint8, np.uint16, np.float32):
        tile, thr = cc.as_image(cc.mask("random_2d_50"), dtype)
        assert tile.dtype == dtype and np.array_equal(co.foreground(tile, thr), cc.mask("random_2d_50"))


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------
def test_python_refusals_need_no_device():
    mask = np.zeros((4, 6), np.uint8)
    with pytest.raises(TypeError, match="uint8, uint16 or float32"):
        _label_ops.label_components(mask.astype(np.int32), 0)
    with pytest.raises(TypeError, match="threshold=None"):
        _label_ops.label_components(mask.astype(np.uint16), None)
    with pytest.raises(ValueError, match="2-D or 3-D"):
        _label_ops.label_components(np.zeros(5, np.uint8), 0)
    for bad in (0, 3):
        with pytest.raises(ValueError, match="connectivity"):
            _label_ops.label_components(mask, 0, connectivity=bad)
    with pytest.raises(ValueError, match="empty"):
        _label_ops.label_components(np.zeros((0, 6), np.uint8), 0)
    t_sim = si.to_spatial_image(np.zeros((2, 4, 6), np.uint8), dims=["t", "y", "x"], scale={"y": 1.0, "x": 1.0}, translation={"y": 0.0, "x": 0.0})
    with pytest.raises(NotImplementedError, match="images\\[1\\]"):
        labels.label_components([lc.label_sim(mask), t_sim])
    with pytest.raises(ValueError, match="no tiles"):
        labels.label_components([])
    with pytest.raises(ValueError, match="one per view"):
        labels.label_components([lc.label_sim(mask)], threshold=[1.0, 2.0])


def test_entry_refuses_bad_arguments_before_any_device():
    """The checks that come before mvs_check_ready: codes, never a crash, on a machine without a GPU too."""
    lib = _lib.load()
    tile = np.zeros((4, 6), np.uint8)
    view, keep = _label_ops.label_view(tile, None, None, 0)
    view.dtype = _lib.MVS_U8
    out, n = np.zeros((4, 6), np.int32), C.c_int64()

    def call(v=view, ndim=2, connectivity=1, out_ptr=out.ctypes.data, mem=_lib.MVS_MEM_HOST, n_ref=C.byref(n)):
        return lib.mvs_label_components(0, None if v is None else C.byref(v), ndim, 0.0, connectivity, 1, C.c_void_p(out_ptr), mem, n_ref)

    assert call(v=None) == -1 and call(out_ptr=None) == -1 and call(n_ref=None) == -1
    assert call(ndim=1) == -1 and call(ndim=4) == -1
    assert call(connectivity=0) == -1 and call(connectivity=3) == -1 and call(ndim=3, connectivity=4) == -1
    assert call(mem=7) == -1
    other = _lib.mvs_view_t.from_buffer_copy(view)
    other.dtype = 3
    assert call(v=other) == _lib.ERR_UNSUPPORTED                          # a dtype other than the three (int32 label tiles among them)
    other = _lib.mvs_view_t.from_buffer_copy(view)
    other.stride[2] = 2
    assert call(v=other) == _lib.ERR_UNSUPPORTED
    other = _lib.mvs_view_t.from_buffer_copy(view)
    other.shape[0] = 2
    assert call(v=other) == -1                                            # a 2D tile with two planes
    other = _lib.mvs_view_t.from_buffer_copy(view)
    other.mem = _lib.MVS_MEM_DEVICE                                       # (nothing is read: the size is refused first)
    other.shape[:] = [1, 46341, 46341]
    other.stride[:] = [46341 * 46341, 46341, 1]
    assert call(v=other) == _lib.ERR_UNSUPPORTED                          # 2^31 + 4 voxels
    assert b"2^31" in lib.mvs_last_error(0)
    del keep


# ---- the driver under a recording stand-in ------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def label_components(self, tile, threshold, connectivity=1, min_voxels=1, device=0, out_on_device=False):
        self.calls.append((tile, threshold, connectivity, min_voxels, device, out_on_device))
        return co.label_components(tile, 0 if threshold is None else threshold, connectivity, min_voxels)


def test_driver_carries_geometry_and_thresholds(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(labels, "_label_ops", rec)
    rng = np.random.default_rng(3)
    tiles = [(rng.random((20, 30)) * 1000).astype(np.uint16) for _ in range(3)]
    sims = [lc.label_sim(tiles[0]), lc.label_sim(tiles[1], origin=(4.5, 22.0), spacing=(1.5, 2.0), affine=lc.rotation(2, 10.0, (3.0, 4.0))),
            lc.label_sim(tiles[2], origin=(100.0, 0.0))]
    si.set_sim_affine(sims[1], np.diag([2.0, 1.0, 1.0]), "other")
    given = [msi_utils.get_msim_from_sim(sims[0])] + sims[1:]
    got = labels.label_components(given, threshold=[100.0, 500.0, 900.0], connectivity=2, min_voxels=3, device=2, keep_on_device=False)
    assert [c[1:] for c in rec.calls] == [(100.0, 2, 3, 2, False), (500.0, 2, 3, 2, False), (900.0, 2, 3, 2, False)]
    assert all(np.array_equal(np.asarray(c[0]), t) for c, t in zip(rec.calls, tiles))
    for res, sim, tile, thr in zip(got, sims, tiles, (100.0, 500.0, 900.0)):
        want, n = co.label_components(tile, thr, 2, 3)
        assert res.data.dtype == np.int32 and np.array_equal(res.data, want) and res.attrs["n_labels"] == n
        assert tuple(res.dims) == ("y", "x")
        assert si.get_origin_from_sim(res) == si.get_origin_from_sim(sim) and si.get_spacing_from_sim(res) == si.get_spacing_from_sim(sim)
        assert set(si.get_tranform_keys_from_sim(res)) == set(si.get_tranform_keys_from_sim(sim))
        for key in si.get_tranform_keys_from_sim(sim):
            assert np.array_equal(np.asarray(si.get_affine_from_sim(res, key)), np.asarray(si.get_affine_from_sim(sim, key)))
    assert "other" in si.get_tranform_keys_from_sim(got[1])
    # one threshold for all views; None for masks
    rec.calls.clear()
    labels.label_components(sims, threshold=250)
    assert [c[1] for c in rec.calls] == [250] * 3 and [c[2:] for c in rec.calls] == [(1, 1, 0, False)] * 3
    rec.calls.clear()
    labels.label_components([lc.label_sim((tiles[0] > 500).astype(np.uint8))], keep_on_device=True)
    assert rec.calls[0][1] is None and rec.calls[0][5] is True


# ---- end to end through the oracles alone -------------------------------------------------------------------------------------------
def test_disc_mosaic_components_then_stitching_through_the_oracles():
    """The disc mosaic as uint16 image tiles, thresholded and labelled per tile by the oracle, stitched by the oracle of label
    stitching: scipy.ndimage.label of the whole mosaic's mask, up to a bijection of the ids, which must exist."""
    truth_mask, sims = cc.disc_image_tiles()
    whole, n_whole = ndimage.label(truth_mask)
    assert n_whole == lc.N_DISCS
    tiles = [co.label_components(np.asarray(s.data), cc.DISC_THRESHOLD)[0] for s in sims]
    label_sims = [s.copy(data=t) for s, t in zip(sims, tiles)]
    counts = [lo.label_counts(t) for t in tiles]
    pairs = labels.view_pairs(label_sims, lc.KEY)
    tables = {(a, b): lc.oracle_pair_table(label_sims[a], label_sims[b]) for a, b in pairs}
    luts, n = lo.match_labels(counts, tables)
    fused = lc.oracle_fuse(label_sims, luts)
    assert n == n_whole and fused.shape == whole.shape and lo.same_up_to_bijection(fused, whole)
    assert not lo.same_up_to_bijection(lc.oracle_fuse(label_sims, None), whole)


# ---- the plan header and the shared union / find on CPU threads -----------------------------------------------------------------------
def build_host_program(tmp_path, sanitizers):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / ("components_host_test_" + sanitizers.replace(",", "_"))
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all", "-I",
           os.path.join(ROOT, "multiview-stitcher_amd", "csrc"), os.path.join(ROOT, "tests", "native", "components_host_test.cpp"), "-o", str(exe)]
    return exe, subprocess.run(cmd, capture_output=True, text=True, timeout=600)


def host_labels(exe, tmp_path, name, connectivity, min_voxels=1, threads=4, per=0):
    m = cc.mask(name)
    path = tmp_path / (name + ".u8")
    path.write_bytes(m.astype(np.uint8).tobytes())
    shape = (1,) * (3 - m.ndim) + m.shape
    r = subprocess.run([str(exe), "label", str(m.ndim), *map(str, shape), str(connectivity), str(min_voxels), str(threads), str(per), str(path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    first, second = r.stdout.strip().splitlines()
    assert first.startswith("N ") and second.startswith("L ")
    return np.array(second.split()[1:], dtype=np.int32).reshape(m.shape), int(first.split()[1])


def test_plan_and_union_find_under_sanitizers(tmp_path):
    exe, r = build_host_program(tmp_path, "address,undefined")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    # half neighbourhoods: 2 / 4 offsets in 2-D and 3 / 9 / 13 in 3-D; nothing out of range
    offsets = {tuple(int(v) for v in ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in lines if ln.startswith("O ")}
    assert offsets == {(2, 0): [0, 0], (2, 1): [2, 1], (2, 2): [4, 1], (2, 3): [0, 0], (3, 0): [0, 0], (3, 1): [3, 2], (3, 2): [9, 4], (3, 3): [13, 4],
                       (3, 4): [0, 0]}
    # the scan partition covers every voxel once, in at most 2048 ranges of a multiple of 256 voxels
    plans = {int(ln.split()[1]): [int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("P ")}
    assert all(p[2] == 1 for p in plans.values()) and len(plans) == 11
    assert plans[1][:2] == [1, 256] and plans[257][:2] == [2, 256] and plans[524288][:2] == [2048, 256] and plans[524289][:2] == [1025, 512]
    assert plans[2**31 - 1][:2] == [2048, 1048576]
    voxels = {tuple(int(v) for v in ln.split()[1:4]): int(ln.split()[4]) for ln in lines if ln.startswith("V ")}
    assert voxels[(512, 512, 512)] == 2**27 and voxels[(1, 1, 2**31 - 1)] == 2**31 - 1 and voxels[(5, 1, 9)] == 45
    assert voxels[(1, 46341, 46341)] == -1 and voxels[(2, 1, 2**30)] == -1 and voxels[(1290, 1291, 1290)] == -1
    # the launches restated on four CPU threads through the shared union / find: the oracle's labels, whatever the chunks per wave
    for name, per in [("serpentine", 0), ("serpentine", 2), ("comb", 0), ("comb", 3), ("nested_u", 0), ("checkerboard", 0), ("row_300", 2),
                      ("random_3d_50", 0), ("random_3d_50", 5), ("volume_5x1x9", 0)]:
        for connectivity in cc.connectivities(name):
            got, n = host_labels(exe, tmp_path, name, connectivity, per=per)
            want, want_n = cc.want(name, connectivity)
            assert n == want_n and np.array_equal(got, want), (name, connectivity, per)
    got, n = host_labels(exe, tmp_path, "random_2d_50", 1, min_voxels=5, per=2)
    want, want_n = cc.want("random_2d_50", 1, 5)
    assert n == want_n and np.array_equal(got, want)


def test_union_find_under_the_thread_sanitizer(tmp_path):
    """The same program under -fsanitize=thread where the compiler and the machine have it: eight threads on the cases with the
    most contended roots."""
    exe, r = build_host_program(tmp_path, "thread")
    if r.returncode != 0:
        pytest.skip("the host compiler has no thread sanitizer: " + r.stderr[-200:])
    probe = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    if probe.returncode != 0 and "ThreadSanitizer" in probe.stderr and "data race" not in probe.stderr:
        pytest.skip("the thread sanitizer does not run here: " + probe.stderr[-200:])
    assert probe.returncode == 0, probe.stderr[-3000:]
    for name in ("serpentine", "comb", "all_foreground", "checkerboard"):
        for connectivity in cc.connectivities(name):
            got, n = host_labels(exe, tmp_path, name, connectivity, threads=8)
            want, want_n = cc.want(name, connectivity)
            assert n == want_n and np.array_equal(got, want), (name, connectivity)
