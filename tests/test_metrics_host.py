"""CPU tests of metrics.tile_pair_image_metrics: ``_metric_ops.pair_moments`` is replaced by the scipy stand-in of
tests/metrics_oracle.py, so the whole public function -- pairs, geometry, modes, levels, channels, summary -- runs without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _metric_ops, metrics, mv_graph
from tests import metrics_oracle as mo
from tests.metrics_helpers import assert_same_structure, make_tile, translation_affine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def on_cpu(monkeypatch):
    """Every call of the moments kernel goes to the oracle's stand-in and is recorded."""
    calls = []

    def stand_in(fixed, moving, fixed_affine, cand_affines, grid_shape, halfspaces=None, device=0):
        calls.append({"fixed": np.asarray(fixed), "moving": np.asarray(moving), "fixed_affine": fixed_affine, "cand_affines": cand_affines,
                      "grid_shape": tuple(grid_shape), "halfspaces": halfspaces})
        return mo.pair_moments(fixed, moving, fixed_affine, cand_affines, grid_shape, halfspaces)

    monkeypatch.setattr(_metric_ops, "pair_moments", stand_in)
    return calls


def textured(shape, seed):
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    return (ndimage.gaussian_filter(rng.random(shape), 1.5) * 4000).astype(np.uint16)


def two_tiles(shift=(0.0, 30.0), extra=None):
    """Two 2D tiles of 40 x 50 px at unit spacing cut from one scene, the second ``shift`` px further (stage key "stage")."""
    scene = textured((60, 120), 3)
    tiles = []
    for s in ((0.0, 0.0), shift):
        y0, x0 = int(s[0]), int(s[1])
        aff = {"stage": translation_affine(s)}
        if extra:
            aff.update({k: translation_affine(np.asarray(s) + (np.asarray(d) if s is shift else 0.0)) for k, d in extra.items()})
        tiles.append(make_tile(scene[y0:y0 + 40, x0:x0 + 50], aff))
    return [t[0] for t in tiles], [t[1] for t in tiles]


# ---- geometry on hand-derived numbers -----------------------------------------------------------------------------------------
def test_comparison_bbox_of_two_shifted_tiles(on_cpu):
    msims, views = two_tiles()
    got = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage")
    assert list(got["pairs"]) == [(0, 1)]
    bb = got["bboxes"][(0, 1)]
    assert np.array_equal(bb["lower"], [0.0, 30.0]) and np.array_equal(bb["upper"], [39.0, 49.0])
    assert on_cpu[0]["grid_shape"] == (40, 20)
    # the same pixels on both sides: NCC 1 up to the rounding of the sums
    assert abs(got["pairs"][(0, 1)]["stage"]["ncc"] - 1.0) < 1e-12
    assert_same_structure(got, mo.tile_pair_image_metrics(views, "stage", ["stage"]))


def test_max_tolerance_shrinks_the_bbox(on_cpu):
    msims, _ = two_tiles()
    bb = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys=["stage"], max_tolerance=2)["bboxes"][(0, 1)]
    assert np.array_equal(bb["lower"], [2.0, 32.0]) and np.array_equal(bb["upper"], [37.0, 47.0])
    bb = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys=["stage"], max_tolerance={"y": 3})["bboxes"][(0, 1)]
    assert np.array_equal(bb["lower"], [3.0, 30.0]) and np.array_equal(bb["upper"], [36.0, 49.0])


def test_pair_without_overlap_after_shrinking_keeps_its_entries(on_cpu):
    """Mode 2 names the pair itself; shrinking each tile by 11 px leaves the 20 px overlap empty."""
    msims, views = two_tiles()
    g = mv_graph.Graph([0, 1])
    g.add_edge(0, 1, transform=np.eye(3))
    got = metrics.tile_pair_image_metrics(msims, "stage", pairs_graph=g, max_tolerance=11)
    assert got["bboxes"] == {(0, 1): None}
    assert np.isnan(got["pairs"][(0, 1)]["transform"]["ncc"]) and np.isnan(got["summary"]["transform"]["ncc"])
    assert not on_cpu
    assert_same_structure(got, mo.tile_pair_image_metrics(views, "stage", pairs_graph={(0, 1): np.eye(3)}, max_tolerance=11))
    # Mode 1 does not see the pair at all (metrics.py:180-182: the adjacency graph takes the same tolerance)
    got = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", max_tolerance=11)
    assert got["pairs"] == {} and np.isnan(got["summary"]["stage"]["ncc"])


def test_bidirectional_gives_both_directions(on_cpu):
    msims, views = two_tiles()
    one = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage")
    both = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", bidirectional=True)
    assert list(one["pairs"]) == [(0, 1)] and list(both["pairs"]) == [(0, 1), (1, 0)]
    # seen from tile 1 the overlap is its first 20 columns
    assert np.array_equal(both["bboxes"][(1, 0)]["lower"], [0.0, 0.0]) and np.array_equal(both["bboxes"][(1, 0)]["upper"], [39.0, 19.0])
    assert_same_structure(both, mo.tile_pair_image_metrics(views, "stage", ["stage"], bidirectional=True))


# ---- the two modes -----------------------------------------------------------------------------------------------------------------
def test_mode_2_takes_the_transform_of_the_edge(on_cpu):
    """Edge transform = world(0) -> world(1), here a translation by (1, -2): p_moving = inv(T_moving_base) @ T_edge @ T_fixed_base
    = translation by (1, -2) + (0, 30) - (0, 30) forwards (grid origin (0, 30) in tile 0).  Backwards (fixed = view 1, T_fixed_base =
    translation by (0, 30), T_moving_base = identity) the reference's expression inv(T_fixed_base) @ inv(T_edge) @ T_moving_base
    (metrics.py:367-368) is the translation by -(0, 30) - (1, -2) = (-1, -28) -- the operands are in the order of the forward
    direction, not inv(T_moving_base) @ inv(T_edge) @ T_fixed_base = (-1, 32); it is kept as it stands."""
    msims, views = two_tiles()
    T_edge = translation_affine([1.0, -2.0])
    g = mv_graph.Graph([0, 1])
    g.add_edge(0, 1, transform=T_edge)
    got = metrics.tile_pair_image_metrics(msims, "stage", pairs_graph=g, bidirectional=True)
    assert list(got["pairs"]) == [(0, 1), (1, 0)] and list(got["summary"]) == ["transform"]
    forward, backward = on_cpu
    # grid index -> moving pixel: the grid starts at the comparison box's lower corner in the fixed tile
    assert np.array_equal(forward["cand_affines"][0][0], np.eye(2)) and np.allclose(forward["cand_affines"][0][1], [0 + 1.0, 30 - 2.0 - 30.0], atol=1e-12)
    assert np.array_equal(backward["cand_affines"][0][0], np.eye(2)) and np.allclose(backward["cand_affines"][0][1], [-1.0, -28.0], atol=1e-12)
    want = mo.tile_pair_image_metrics(views, "stage", pairs_graph={(0, 1): T_edge}, bidirectional=True)
    assert_same_structure(got, want)
    for p in want["pairs"]:
        assert np.isclose(got["pairs"][p]["transform"]["ncc"], want["pairs"][p]["transform"]["ncc"], rtol=0, atol=1e-12, equal_nan=True)
    # (under the reference's reverse expression tile 0 lies wholly outside the grid: no sample pair)
    assert 0.5 < got["pairs"][(0, 1)]["transform"]["ncc"] < 1.0 and np.isnan(got["pairs"][(1, 0)]["transform"]["ncc"])
    # a networkx-style graph: .nodes(), .edges(), .edges[i, j]
    class View(dict):
        def __call__(self):
            return list(self)

    class G:
        nodes = View({0: {}, 1: {}})
        edges = View({(0, 1): {"transform": T_edge}})

    assert metrics.tile_pair_image_metrics(msims, "stage", pairs_graph=G())["pairs"][(0, 1)] == got["pairs"][(0, 1)]


def test_exactly_one_selector(on_cpu):
    msims, _ = two_tiles()
    g = mv_graph.Graph([0, 1])
    g.add_edge(0, 1, transform=np.eye(3))
    with pytest.raises(ValueError, match="Exactly one of 'query_transform_keys' or 'pairs_graph'"):
        metrics.tile_pair_image_metrics(msims, "stage")
    with pytest.raises(ValueError, match="Exactly one of 'query_transform_keys' or 'pairs_graph'"):
        metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", pairs_graph=g)


def test_query_keys_are_compared_on_the_same_grid(on_cpu):
    """Two keys: the stage, and the stage with tile 1 off by 1.5 px.  One kernel call with both candidates, the better key wins."""
    msims, views = two_tiles(extra={"off": (0.0, 1.5)})
    got = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys=["stage", "off"])
    assert len(on_cpu) == 1 and len(on_cpu[0]["cand_affines"]) == 2
    want = mo.tile_pair_image_metrics(views, "stage", ["stage", "off"])
    assert_same_structure(got, want)
    for q in ("stage", "off"):
        assert abs(got["pairs"][(0, 1)][q]["ncc"] - want["pairs"][(0, 1)][q]["ncc"]) < 1e-12
        assert abs(got["summary"][q]["ncc"] - want["summary"][q]["ncc"]) < 1e-12
    assert got["summary"]["stage"]["ncc"] > got["summary"]["off"]["ncc"]


def test_custom_metric_gets_the_reference_arrays(on_cpu, monkeypatch):
    """A callable that is not the built-in NCC receives float32 arrays, the fixed one NaN outside the halfspaces.  (resample_array
    is replaced by scipy here; tests/test_metrics_gpu.py runs the real one.)"""
    seen = []

    def mean_abs_diff(a, b):
        seen.append((a, b))
        return np.nanmean(np.abs(a - b))

    monkeypatch.setattr(metrics, "resample_array", lambda data, matrix, offset, shape, order, cval, device, out_on_device:
                        mo.sample(np.asarray(data), matrix, offset, shape))
    msims, views = two_tiles(extra={"off": (0.0, 1.5)})
    funcs = {"ncc": metrics.normalized_cross_correlation, "mad": mean_abs_diff}
    got = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys=["off"], metric_funcs=funcs)
    want = mo.tile_pair_image_metrics(views, "stage", ["off"], metric_funcs={"ncc": mo.normalized_cross_correlation, "mad": lambda a, b: np.nanmean(np.abs(a - b))})
    assert_same_structure(got, want)
    (a, b), = seen
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == (40, 20)
    assert abs(got["pairs"][(0, 1)]["off"]["mad"] - want["pairs"][(0, 1)]["off"]["mad"]) < 1e-12
    # a function called normalized_cross_correlation of the reference's module selects the kernel as well
    ref_ncc = lambda a, b: 0.0
    ref_ncc.__name__, ref_ncc.__module__ = "normalized_cross_correlation", "multiview_stitcher.metrics"
    n = len(on_cpu)
    assert metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys=["off"], metric_funcs={"x": ref_ncc})["pairs"][(0, 1)]["off"]["x"] \
        == got["pairs"][(0, 1)]["off"]["ncc"]
    assert len(on_cpu) == n + 1 and len(seen) == 1


# ---- summary -----------------------------------------------------------------------------------------------------------------------
def test_summary_is_weighted_by_overlap_volume():
    pairs = {(0, 1): {"q": {"ncc": 0.5}}, (0, 2): {"q": {"ncc": np.nan}}, (1, 2): {"q": {"ncc": 1.0}}}
    vols = {(0, 1): 1.0, (0, 2): 2.0, (1, 2): 3.0}
    assert metrics.summarize(pairs, vols, ["q"], ["ncc"]) == {"q": {"ncc": (0.5 * 1 + 1.0 * 3) / 4}}
    nan = {p: {"q": {"ncc": np.nan}} for p in pairs}
    assert np.isnan(metrics.summarize(nan, vols, ["q"], ["ncc"])["q"]["ncc"])


# ---- resolution level and channel ------------------------------------------------------------------------------------------------
def test_spacing_picks_the_level_per_pair_and_channel_by_coordinate(on_cpu):
    scene = np.stack([textured((60, 120), 5), textured((60, 120), 6)])
    msims = [make_tile(scene[:, :40, x0:x0 + 50], {"stage": translation_affine((0.0, float(x0)))}, scale_factors=[2], c_coords=["dapi", "gfp"])[0]
             for x0 in (0, 30)]
    metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage")
    assert on_cpu[-1]["fixed"].shape == (40, 50) and np.array_equal(on_cpu[-1]["fixed"], scene[0, :40, :50])       # level 0, first channel
    metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", metric_channel="gfp")
    assert np.array_equal(on_cpu[-1]["fixed"], scene[1, :40, :50]) and np.array_equal(on_cpu[-1]["moving"], scene[1, :40, 30:80])
    # spacing 2 without a level: scale1 (spacing 2) is the coarsest level that is still fine enough; the box comes from scale0
    got = metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", spacing={"y": 2.0, "x": 2.0})
    assert on_cpu[-1]["fixed"].shape == (20, 25) and on_cpu[-1]["grid_shape"] == (20, 10)
    assert np.array_equal(got["bboxes"][(0, 1)]["lower"], [0.0, 30.0])
    # spacing 1.5: only scale0 is fine enough
    metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", spacing={"y": 1.5, "x": 1.5})
    assert on_cpu[-1]["fixed"].shape == (40, 50) and on_cpu[-1]["grid_shape"] == (27, 13)
    # an explicit level wins: geometry and data of scale1, grid at the given spacing
    metrics.tile_pair_image_metrics(msims, "stage", query_transform_keys="stage", spacing={"y": 4.0, "x": 4.0}, input_res_level=1)
    assert on_cpu[-1]["fixed"].shape == (20, 25)


# ---- the host NCC ------------------------------------------------------------------------------------------------------------------
def test_normalized_cross_correlation_on_arrays():
    nan = np.nan
    assert np.isnan(metrics.normalized_cross_correlation([1.0, nan, 3.0], [nan, 2.0, 5.0]))          # one valid position
    assert np.isnan(metrics.normalized_cross_correlation([2.0, 2.0, 2.0, nan], [1.0, 5.0, 3.0, 4.0]))   # constant image
    # valid positions 0, 1, 3: a = (1, 2, 6), b = (2, 1, 6): a_c = (-2, -1, 3), b_c = (-1, -2, 3) -> 13 / 14
    assert metrics.normalized_cross_correlation([1.0, 2.0, nan, 6.0], [2.0, 1.0, 9.0, 6.0]) == pytest.approx(13.0 / 14.0, abs=1e-15)
    assert metrics.normalized_cross_correlation(np.array([[1, 2], [3, 4]], np.uint8), np.array([[4, 3], [2, 1]], np.uint8)) == pytest.approx(-1.0, abs=1e-15)
    m = mo.moments([1.0, 2.0, nan, 6.0], [2.0, 1.0, 9.0, 6.0])
    assert _metric_ops.ncc_from_moments(m) == pytest.approx(13.0 / 14.0, abs=1e-15)
    assert np.isnan(_metric_ops.ncc_from_moments([1, 5.0, 5.0, 0.0, 0.0, 0.0])) and np.isnan(_metric_ops.ncc_from_moments([9, 5.0, 5.0, 0.0, 3.0, 0.0]))


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
def test_pair_moments_is_exported_declared_and_refuses_bad_arguments():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvs_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mvs_pair_moments\s*\(", text)
    for name in ("MVS_PAIR_MOMENTS_LEN", "MVS_PAIR_MAX_CANDIDATES", "MVS_PAIR_MAX_HALFSPACES", "MVS_PAIR_BLOCK_VOXELS", "MVS_PAIR_MAX_BLOCKS"):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1)) == getattr(_lib, name)
    lib = _lib.load()
    assert hasattr(lib, "mvs_pair_moments") and "mvs_pair_moments" in _lib.SIGNATURES
    # argument checks come before any device work: error codes, never a crash
    v = _lib.mvs_view_t()
    out = np.zeros(6)
    dp = ctypes.POINTER(ctypes.c_double)
    eye, zero = np.eye(3).reshape(9), np.zeros(3)
    args = lambda k, ndim, shape: (0, ctypes.byref(v), ctypes.byref(v), k, eye.ctypes.data_as(dp), zero.ctypes.data_as(dp), ndim, _lib.i64x3(shape), None, 0,
                                   out.ctypes.data_as(dp))
    assert lib.mvs_pair_moments(*args(1, 4, (1, 4, 4))) == -1
    assert lib.mvs_pair_moments(*args(0, 2, (1, 4, 4))) == -1 and lib.mvs_pair_moments(*args(9, 2, (1, 4, 4))) == -1
    assert lib.mvs_pair_moments(*args(1, 2, (2, 4, 4))) == -1
    assert lib.mvs_pair_moments(*args(1, 2, (1, 4, 4))) == -1                   # views without data


# ---- the reduction of csrc/mvs_pair_metrics_dev.h on the host -------------------------------------------------------------------
def test_reduction_header_keeps_the_variance_of_a_camera_offset(tmp_path):
    """The kernel's launch structure replayed on the CPU (tests/native/pair_moments_host_test.cpp) over 16-bit values at 60000 +- 6:
    the moments equal the two-pass float64 ones to rounding (raw sums of squares in float32 would lose them altogether), a constant
    image has M2 == 0 exactly, and so it does through 2048 records and a second step of the grid-stride loop."""
    import shutil
    import subprocess

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "pair_moments_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "pair_moments_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"
    moments = {int(ln.split()[1]): np.array([float(v) for v in ln.split()[3:]]) for ln in lines if ln.startswith("M ")}
    samples = np.array([[float(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("S ")])
    assert len(samples) == 3 * 256 + 5
    want = mo.moments(samples[:, 0], samples[:, 1])
    assert moments[0][0] == want[0] < len(samples)                       # NaN samples do not count
    # n <= 1e3 terms of exact differences: sums good to n 2^-53 relative, 1e-12 leaves a factor of ten
    np.testing.assert_allclose(moments[0][1:], want[1:], rtol=1e-12, atol=0)
    assert abs(_metric_ops.ncc_from_moments(moments[0]) - mo.normalized_cross_correlation(samples[:, 0], samples[:, 1])) < 1e-12
    for variant in (1, 2):
        assert moments[variant][1] == 60123.0 if variant == 1 else moments[variant][0] > 2048 * 256 * 0.98
    assert moments[1][3] == 0.0 and moments[1][5] == 0.0 and moments[1][4] > 0 and np.isnan(_metric_ops.ncc_from_moments(moments[1]))
    # variant 2: integer-and-a-half values over 2048 records; var = E[(c + h/2)^2] of two uniform draws on -6..6: 14 + 14/4
    assert abs(moments[2][3] / moments[2][0] - 17.5) < 0.1 and abs(moments[2][1] - 60000.0) < 0.02
