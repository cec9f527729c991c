"""CPU: the multi-band fusion without a device -- the invariants of its definition on the numpy restatement (tests/multiband_oracle.py),
the conditioning of every input the GPU tests use, ``required_overlap``, the refusals of the C ABI that need no device, and
csrc/mvs_multiband_plan.h compiled for the host under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, fusion, multiband
from tests import multiband_cases as mc
from tests import multiband_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

U8_DIFFER_CAP = mc.U8_DIFFER_CAP


def _box(whole, lo, hi):
    return whole[tuple(slice(a, b) for a, b in zip(lo, hi))]


FRAME_2D = (-7, 5)          # the whole stack's own index_origin: chunk starts of both parities, negative ones among them
BOXES_2D = [((10, 11), (45, 60)), ((0, 0), (33, 47)), ((35, 40), (70, 90)), ((34, 45), (61, 78))]


@pytest.mark.parametrize("n_levels", [1, 2, 3])
def test_chunked_equals_whole_stack_2d(n_levels):
    V, B = mc.make_views((70, 90), 2, 1)
    whole = mo.multi_band(V, B, n_levels, FRAME_2D)
    halo = mo.radius(n_levels)
    starts = set()
    for lo, hi in BOXES_2D:
        for clip in (True, False):
            got = mo.chunked(V, B, n_levels, lo, hi, halo, FRAME_2D, clip=clip)
            assert np.array_equal(got, _box(whole, lo, hi)), (lo, hi, clip)
            starts.update((f + (max(0, l - halo) if clip else l - halo)) for f, l in zip(FRAME_2D, lo))
    assert any(s < 0 for s in starts) and {s % 2 for s in starts} == {0, 1}


def test_chunked_equals_whole_stack_3d():
    V, B = mc.make_views((6, 40, 44), 3, 2)
    levels, frame = {"z": 1, "y": 2, "x": 2}, (3, -9, 4)
    halo = [mo.radius(1), mo.radius(2), mo.radius(2)]
    whole = mo.multi_band(V, B, levels, frame)
    for lo, hi in [((0, 7, 9), (6, 25, 30)), ((2, 16, 15), (5, 40, 44)), ((1, 0, 20), (4, 21, 33))]:
        for clip in (True, False):
            assert np.array_equal(mo.chunked(V, B, levels, lo, hi, halo, frame, clip=clip), _box(whole, lo, hi)), (lo, hi, clip)


@pytest.mark.parametrize("n_levels", [1, 2, 3])
def test_smaller_halo_or_unanchored_chunk_differs(n_levels):
    """The radius is sharp next to a seam of the winner map (views that disagree everywhere), and the anchoring matters at an odd
    start."""
    V, B = mc.make_views((70, 90), 2, 1, full=True)
    whole = mo.multi_band(V, B, n_levels, FRAME_2D)
    halo = mo.radius(n_levels)
    # (the full radius is reached only from rows that are even at every level: global row 30 = 6 (mod 8) looks 4 (2^L - 1) rows up)
    for lo in [(37, 43), (29, 44)]:
        assert (FRAME_2D[0] + lo[0]) % 8 == 6
        got = mo.chunked(V, B, n_levels, lo, (70, 90), halo - 1, FRAME_2D, clip=True)
        assert not np.array_equal(got, _box(whole, lo, (70, 90))), lo
        assert np.array_equal(mo.chunked(V, B, n_levels, lo, (70, 90), halo, FRAME_2D, clip=True), _box(whole, lo, (70, 90))), lo
    lo = (halo + 8, halo + 6)          # the chunk starts at the odd global index frame + lo - halo; anchored at 0 it decimates the other lattice
    assert (FRAME_2D[0] + lo[0] - halo) % 2 == 1
    got = mo.chunked(V, B, n_levels, lo, (70, 90), halo, FRAME_2D, clip=True, anchored=False)
    assert not np.array_equal(got, _box(whole, lo, (70, 90)))


def test_identical_views_give_f0():
    V, B = mc.make_views((40, 50), 3, 5)
    V = np.stack([np.where(np.isfinite(v), np.nan_to_num(V[0], nan=101.5), np.nan) for v in V]).astype(np.float32)
    F0, _, _, cov = mo.pointwise(V, B)
    got = mo.multi_band(V, B, 3)
    assert np.abs(got - np.where(cov, F0, 0.0)).max() <= 1e-12 * np.abs(F0).max()


def test_zero_levels_is_the_hard_seam():
    V, B = mc.make_views((40, 50), 3, 6)
    _, _, winner, cov = mo.pointwise(V, B)
    hard = np.where(cov, np.take_along_axis(np.nan_to_num(V.astype(np.float64)), winner[None], axis=0)[0], 0.0)
    got = mo.multi_band(V, B, 0)
    assert np.abs(got - hard).max() <= 1e-12 * np.abs(hard).max()
    assert np.array_equal(got == 0, ~cov)


@pytest.mark.parametrize("n_levels", [1, 3])
def test_single_view_regions_away_from_overlaps_equal_that_view(n_levels):
    from scipy import ndimage

    V, B = mc.make_views((70, 90), 2, 1)
    finite = np.isfinite(V)
    overlap = finite.sum(0) >= 2
    r = mo.radius(n_levels)
    near = ndimage.binary_dilation(overlap, structure=np.ones((2 * r + 1, 2 * r + 1), bool))
    got = mo.multi_band(V, B, n_levels)
    checked = 0
    for v in range(2):
        sel = finite[v] & ~near & (finite.sum(0) == 1)
        assert np.array_equal(got[sel], V[v].astype(np.float64)[sel])
        checked += int(sel.sum())
    assert checked > 400


@pytest.mark.parametrize("name", sorted(mc.float_cases()))
def test_gpu_inputs_are_well_conditioned(name):
    """The restatement in float32 against itself in float64 stays within HALF the float bar on every input of the GPU tests."""
    V, B, n_levels, origin = mc.float_cases()[name]
    want = mo.multi_band(V, B, n_levels, origin)
    low = mo.multi_band(V, B, n_levels, origin, dtype=np.float32)
    assert np.isfinite(want).all()
    assert np.all(np.abs(low - want) <= 0.5 * mc.float_bar(want))


def test_u8_input_overshoots_and_is_stable_under_float32():
    V, B, n_levels = mc.checker_u8()
    want = mo.multi_band(V, B, n_levels)
    assert want.min() < -5 and want.max() > 260                # the bands leave the range at both ends
    a, b = mo.cast(want, np.uint8), mo.cast(mo.multi_band(V, B, n_levels, dtype=np.float32), np.uint8)
    assert (a == 0).any() and (a == 255).any()
    assert np.abs(a.astype(int) - b.astype(int)).max() <= 1
    assert (a != b).mean() <= U8_DIFFER_CAP


def test_cast_rounds_half_to_even_and_saturates():
    vals = np.array([-3.0, -0.5, 0.5, 1.5, 2.5, 254.5, 255.5, 300.0, 65535.5, 1e9])
    assert mo.cast(vals, np.uint8).tolist() == [0, 0, 0, 2, 2, 254, 255, 255, 255, 255]
    assert mo.cast(vals, np.uint16).tolist() == [0, 0, 0, 2, 2, 254, 256, 300, 65535, 65535]
    assert mo.cast(vals, np.float32).dtype == np.float32


def test_required_overlap_values():
    ro = fusion.multi_band_fusion.required_overlap
    assert ro(None) == 28 and ro({}) == 28                     # n_levels defaults to 3
    assert [ro({"n_levels": n}) for n in range(7)] == [0, 4, 12, 28, 60, 124, 252]
    assert ro({"n_levels": {"z": 1, "y": 2, "x": 3}}) == {"z": 4, "y": 12, "x": 28}
    assert all(isinstance(ro({"n_levels": n}), int) for n in range(7))
    # through fuse()'s halo rule: raised to the function's requirement per dim
    assert fusion._halo_overlap(2, ["y", "x"], [(None, None), (fusion.multi_band_fusion, {"n_levels": 2})], None) == {"y": 12, "x": 12}
    assert fusion._halo_overlap(None, ["z", "y", "x"], [(fusion.multi_band_fusion, {"n_levels": {"z": 0, "y": 1, "x": 2}})], None) == {"z": 0, "y": 4, "x": 12}
    assert fusion.builtin("multi_band_fusion") is fusion.multi_band_fusion is multiband.multi_band_fusion


def test_level_arguments():
    assert multiband._levels3(3, 2) == [0, 3, 3] and multiband._levels3({"z": 1, "y": 2, "x": 0}, 3) == [1, 2, 0]
    assert multiband._origin3(None, 3) == [0, 0, 0] and multiband._origin3((-12, 23), 2) == [0, -12, 23]
    assert multiband._origin3({"y": 4, "x": -1}, 2) == [0, 4, -1]
    for bad in (7, -1, 1.5, {"y": 1}, {"z": 1, "y": 1, "x": 1}):
        with pytest.raises(ValueError):
            multiband._levels3(bad, 2)
    with pytest.raises(ValueError):
        multiband._origin3((1, 2, 3), 2)
    with pytest.raises(ValueError):
        multiband._origin3((0.5, 2), 2)


def test_abi_refusals_need_no_device():
    lib = _lib.load()
    assert C.sizeof(_lib.mvs_multiband_opts_t) == 16 + 24 + 24 + 8       # 3 x int32 (+ padding), 2 x 3 x int64, 2 x int32
    data = np.zeros((2, 1, 8, 8), np.float32)
    out = np.zeros((1, 8, 8), np.float32)

    def call(n_views=2, ndim=2, levels=(0, 1, 1), shape=(1, 8, 8)):
        opts = _lib.mvs_multiband_opts_t()
        for k in range(3):
            opts.levels[k] = levels[k]
        opts.out_dtype = _lib.MVS_F32
        return lib.mvs_multiband_fuse(0, C.c_void_p(data.ctypes.data), C.c_void_p(data.ctypes.data), n_views, _lib.i64x3(shape), ndim, C.byref(opts),
                                      C.c_void_p(out.ctypes.data), _lib.MVS_MEM_HOST)

    assert call(n_views=0) == _lib.ERR_UNSUPPORTED
    assert call(n_views=255) == _lib.ERR_UNSUPPORTED
    assert call(ndim=1) == _lib.ERR_UNSUPPORTED and call(ndim=4) == _lib.ERR_UNSUPPORTED
    assert call(levels=(0, -1, 1)) == _lib.ERR_UNSUPPORTED
    assert call(levels=(0, 1, 7)) == _lib.ERR_UNSUPPORTED
    assert call(levels=(1, 1, 1)) < 0 and call(shape=(1, 0, 8)) < 0      # 2D data with a z level / an empty axis: refused as well
    assert lib.mvs_multiband_fuse(0, None, None, 2, _lib.i64x3((1, 8, 8)), 2, None, None, _lib.MVS_MEM_HOST) < 0


def test_fuse_np_refuses_a_weights_func_before_touching_the_device():
    import inspect

    src = inspect.getsource(fusion.fuse_np)
    assert src.index("multi_band_fusion cannot be combined with a weights_func") < src.index("_fuse_np_multiband(")


def test_plan_header_under_sanitizers(tmp_path):
    """tests/native/multiband_plan_host_test.cpp: a stand-alone program of mvs_multiband_plan.h, built with the host compiler and
    -fsanitize=address,undefined and run directly; its extents and starts equal the restatement's for starts -13..13, lengths 1..40."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    assert cxx is not None, "no host C++ compiler"
    exe = tmp_path / "multiband_plan_host_test"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "multiband_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    seen = 0
    for ln in lines:
        if not ln.startswith("A "):
            continue
        vals = [int(v) for v in ln.split()[1:]]
        start, n, levels, top = vals[:4]
        got = list(zip(vals[4::2], vals[5::2]))
        assert got == mo.axis_geometry(start, n, levels, top), ln
        seen += 1
    assert seen == 27 * 40 * 3
    facts = dict(ln.split()[1:3] for ln in lines if ln.startswith("F "))
    assert facts == {"max_levels": "6", "max_views": "254", "tile_y": "16", "tile_x": "32", "lds_bytes": "13668", "bad_plans_refused": "1",
                     "storage_2d_ok": "1", "storage_3d_ok": "1", "grid_capped": "1"}
    assert (2 * int(facts["tile_y"]), 2 * int(facts["tile_x"])) == mc.REDUCE_TILE
