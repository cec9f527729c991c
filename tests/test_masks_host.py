"""CPU: the host side of the sample masks (masks.py): the Otsu arithmetic shared with mv_graph.threshold_otsu, the pair list of a
contact matrix, the coordinates of masks under binning, the reference-name wrappers, the refusals that need no device, and
csrc/mvs_masks_plan.h compiled for the host under the address and undefined-behaviour sanitizers."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _mask_ops, masks, mv_graph, registration
from multiview_stitcher_amd import spatial_image_utils as si
from oracle import resolve_oracle as ro
from tests import masks_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _samples():
    rng = np.random.default_rng(3)
    return {
        "bimodal": np.concatenate([rng.normal(100.0, 10.0, 4000), rng.normal(400.0, 30.0, 1500)]),
        "constant_plus_outlier": np.r_[np.full(999, 7.0), 1000.0],
        "two_valued": np.r_[np.full(300, 2.0), np.full(200, 5.0)],
        "uint16_like": rng.integers(0, 65536, 5000).astype(np.float64),
    }


@pytest.mark.parametrize("name", sorted(_samples()))
def test_otsu_from_histogram_is_threshold_otsu(name):
    v = _samples()[name]
    counts, _ = np.histogram(v, 256, (v.min(), v.max()))
    want = mv_graph.threshold_otsu(v)
    assert masks.otsu_from_histogram(counts, v.min(), v.max()) == want
    assert masks.otsu_from_histogram(counts.astype(np.uint64), v.min(), v.max()) == want      # the kernel's counts are uint64
    assert want == ro.threshold_otsu(v)             # sharing the arithmetic did not change threshold_otsu
    assert masks.otsu_from_histogram is mv_graph.otsu_from_histogram


def test_pair_list_from_a_counts_matrix():
    counts = np.zeros((5, 5), dtype=np.uint64)
    counts[0, 3] = 2
    counts[1, 2] = 1
    counts[0, 1] = 7
    counts[4, 4] = 9            # the diagonal and the lower triangle are not pairs
    counts[3, 1] = 5
    assert masks.pairs_from_counts(counts) == [(0, 1), (0, 3), (1, 2)]
    assert masks.pairs_from_counts(np.zeros((3, 3), dtype=np.uint64)) == []
    assert mo.pairs_of(counts) == [(0, 1), (0, 3), (1, 2)]


def test_mask_coordinates_under_binning():
    """A mask of a binned tile sits on the coordinates ``registration._binned_coords`` gives: the mean of every full group."""
    coords = 10.0 + 0.5 * np.arange(11)
    got = registration._binned_coords(coords, 3)
    assert np.array_equal(got, np.array([10.5, 12.0, 13.5]))          # 11 // 3 groups, the trailing two samples dropped
    sim = si.to_spatial_image(np.zeros((4, 11), np.uint16), dims=["y", "x"], scale={"y": 2.0, "x": 0.5}, translation={"y": -1.0, "x": 10.0})
    assert registration._bin_sim(sim, {"y": 1, "x": 1}, 0) is sim     # no binning: the tile itself, no device touched
    assert masks._per_axis({"x": 3}, ["y", "x"], "binning") == [0, 3]
    assert masks._per_axis(2, ["z", "y", "x"], "dilate") == [2, 2, 2]
    with pytest.raises(ValueError):
        masks._per_axis([1, 2, 3], ["y", "x"], "dilate")


def test_reference_name_wrappers_signatures():
    p = inspect.signature(registration.get_pairs_from_sample_masks).parameters
    assert list(p)[:3] == ["mask_sims", "transform_key", "fused_mask_spacing"]
    assert p["transform_key"].default == "affine_manual" and p["fused_mask_spacing"].default is None and p["device"].default == 0
    p = inspect.signature(mv_graph.get_connected_labels).parameters
    assert list(p)[:2] == ["labels", "structure"] and p["structure"].default is None
    assert "superset" in mv_graph.get_connected_labels.__doc__
    p = inspect.signature(masks.sample_masks).parameters
    assert list(p)[:7] == ["msims_or_sims", "threshold", "binning", "sigma", "dilate", "device", "keep_on_device"]
    assert list(inspect.signature(masks.otsu_threshold).parameters) == ["msims_or_sims", "n_bins", "sigma", "binning", "device"]
    assert list(inspect.signature(masks.fuse_labels).parameters) == ["mask_sims", "transform_key", "spacing", "device", "output_on_backend"]
    assert list(inspect.signature(masks.contact_pairs).parameters)[:4] == ["labels", "connectivity", "return_counts", "device"]


def _sim(dims, shape):
    sdims = [d for d in dims if d in "zyx"]
    return si.to_spatial_image(np.zeros(shape, np.uint8), dims=dims, scale={d: 1.0 for d in sdims}, translation={d: 0.0 for d in sdims})


@pytest.mark.parametrize("dim", ["t", "c"])
def test_sims_with_t_or_c_dims_are_refused_by_name(dim):
    sim = _sim([dim, "y", "x"], (1, 4, 5))
    for call in (lambda: masks.sample_masks([sim], threshold=1.0), lambda: masks.otsu_threshold([sim]),
                 lambda: masks.fuse_labels([sim], "affine_manual"), lambda: registration.get_pairs_from_sample_masks([sim])):
        with pytest.raises(ValueError, match=f"'{dim}' dim"):
            call()


def test_limits_are_refused_without_a_device():
    sim = _sim(["y", "x"], (4, 5))
    with pytest.raises(ValueError, match="4096"):
        masks.otsu_threshold([sim], n_bins=4097)
    with pytest.raises(ValueError, match="4096"):
        _mask_ops.histogram([sim.data], 4097, 0.0, 1.0)
    with pytest.raises(ValueError, match="32"):
        masks.sample_masks([sim], threshold=1.0, dilate=33)
    with pytest.raises(ValueError, match="32"):
        masks.sample_masks([sim], threshold=1.0, dilate={"x": 40})
    labels = np.zeros((4, 5), np.int32)
    labels[0, 0] = 2049
    with pytest.raises(ValueError, match="2048"):
        masks.contact_pairs(labels)
    with pytest.raises(ValueError, match="2048"):
        mv_graph.get_connected_labels(labels, np.ones((3, 3)))
    assert (_lib.MVS_HIST_MAX_BINS, _lib.MVS_MASK_MAX_DILATE, _lib.MVS_LABEL_MAX) == (4096, 32, 2048)


def test_entry_points_return_unsupported_above_their_limits():
    """The C entries check their limits before they need a device: MVS_ERR_UNSUPPORTED, never a crash."""
    lib = _lib.load()
    view = _lib.mvs_view_t()
    data = np.zeros((1, 4, 16), np.uint8)
    view.data, view.dtype, view.mem = data.ctypes.data, _lib.MVS_U8, _lib.MVS_MEM_HOST
    view.shape[:] = data.shape
    view.stride[:] = [64, 16, 1]
    edges = np.linspace(0.0, 1.0, 4098)
    counts = np.zeros(4097, np.uint64)
    assert lib.mvs_tile_histogram(0, C.byref(view), 1, 4097, edges.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  None, None, None) == _lib.ERR_UNSUPPORTED
    out = np.zeros(data.shape, np.uint8)
    assert lib.mvs_mask_threshold(0, C.byref(view), 3, 0.5, (C.c_int32 * 3)(0, 0, 33), C.c_void_p(out.ctypes.data), None) == _lib.ERR_UNSUPPORTED
    big = np.zeros(1, np.uint64)
    assert lib.mvs_label_contacts(0, C.c_void_p(data.ctypes.data), 3, _lib.i64x3(data.shape), 2049, 3,
                                  big.ctypes.data_as(C.POINTER(C.c_uint64))) == _lib.ERR_UNSUPPORTED


def test_plan_header_under_sanitizers(tmp_path):
    """tests/native/masks_plan_host_test.cpp: a stand-alone program of mvs_masks_plan.h, built with the host compiler and
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "masks_plan_host_test"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "masks_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    offsets = {tuple(int(v) for v in ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in lines if ln.startswith("O ")}
    want = {(2, 1): 2, (2, 2): 4, (3, 1): 3, (3, 2): 9, (3, 3): 13}
    for key, (count, bad) in offsets.items():
        assert count == want.get(key, 0), key          # (connectivity 0, 4, and 3 in 2D are out of range: no offsets)
        assert bad == 0, key
        if key in want:
            assert count == len(mo.half_neighbourhood(*key))
    assert set(want) <= set(offsets)

    geometry = {int(ln.split()[1]): [int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("G ")}
    # nx: groups of 16 voxels, padded pitch, workgroups of 256 lanes over nx rows of groups, workgroups of 4 waves over nx rows of 64-voxel chunks
    assert geometry[1] == [1, 16, 1, 1]
    assert geometry[63] == [4, 64, 1, 16]
    assert geometry[64] == [4, 64, 1, 16]
    assert geometry[65] == [5, 80, 2, 33]            # 65 rows x 5 groups = 325 lanes; 65 rows x 2 chunks = 130 waves
    assert geometry[16] == [1, 16, 1, 4] and geometry[17] == [2, 32, 1, 5] and geometry[70] == [5, 80, 2, 35]
    assert geometry[4096][2:] == [2048, 2048] and geometry[4097][:2] == [257, 4112]      # the grid cap
    assert geometry[0][2:] == [1, 2048]              # never an empty grid

    for ln in lines:
        if ln.startswith("H "):
            rows, max_nx, blocks, voxels = (int(v) for v in ln.split()[1:])
            assert 1 <= blocks < 2 ** 31 and voxels < 2 ** 32, ln       # a workgroup's uint32 bins cannot overflow
            assert blocks * (voxels // max_nx) >= rows, ln               # the grid covers every row
