"""GPU: the generic affine fuse kernel ``fuse_kernel<TIn, TOut, ORDER, FUSION, DCT>`` (csrc/mvs_fuse.hip) against the oracle's fuse_np
on chunks whose views carry a real matrix (tests/affine_cases.py; tests/test_affine_cases_host.py proves on the CPU that every case
reaches what it is listed for here).  No option forces the kernel: a view whose pixel matrix is not the identity sends the whole chunk
to it, and the chunk counters say so.  The branches of the kernel and of what it calls, and the cases that reach them:

  brick layout           4 x 4 x 64 (3D): fan3d_12, knife_rot90_3d, mirror_swap, shear_aniso, trimmed, far_origin;
                         1 x 16 x 64 (bz == 1, 2D): fan2d_12, fan2d_70, knife_rot90_2d
  brick_hits_view        turns through every multiple of 30 degrees (fan*_12) and of 360 / 70 (fan2d_70), permutations and mirrors
                         (mirror_swap), shear with a negative determinant and a view that meets the chunk with a corner only
                         (shear_aniso), bricks of a trimmed chunk (lo / hi carry the trim: trimmed)
  cull batches           base = 0 only: every case but fan2d_70; base = 64 with active views: fan2d_70 (70 views on a voxel)
  blend_weight<true>     the first 8 active views of a brick (table in LDS): every weighted_average cell
  blend_weight<false>    the 9th and later active view (table in global memory): fan3d_12, fan2d_12, fan2d_70
  in-bounds test         coordinates an integer -+ k * 1e-10 at the view borders: knife_rot90_2d / _3d under max and simple_average, where a
                         misclassified voxel changes the value by whole counts and the zero mask is compared voxel for voxel;
                         coordinates equal to 0.0 and n - 1: mirror_swap
  sample_view<.., 1>     second tap mirrored to n - 2 with weight 0, NaN there poisons the sample: mirror_swap float32
  sample_view<.., 0>     order 0 under a real matrix: every case but fan2d_70, shear_aniso and far_origin
  wa_update / wa_result  one contributor (exact), two, up to 70: the fans; max and simple_average: knife_rot90, mirror_swap, shear_aniso,
                         trimmed, far_origin
  store_row4             vector branch: the rows that start on a multiple of 4 elements (every fourth row of an odd width, every second
                         one of a width with width % 4 == 2); scalar branch on the other rows and on the row tail: trimmed (width 57),
                         shear_aniso (63), fan3d_12 (77), fan2d_12 (83), fan2d_70 (46), knife_rot90 (90, 78)
  TIn / TOut             uint16, uint8, float32: the fans; uint8: mirror_swap
  DCT = true             more than 8 views (fan2d_12) and a sheared 3D view (shear_aniso) through mvs_fuse_chunk_dct
  mvs_view_to_chunk_frame    chunk and slab shifts folded into the offsets of turned views: the chunked fuse() of fan3d_12
  offsets near 1e5       far_origin

Parity is ``helpers.assert_fused_close`` at its defaults: float32 within 1e-4 relative, integers within one count and only next to an
integer boundary of the reference's float result, the reference's own noise floor on at most 1 % of the voxels."""
import numpy as np
import pytest

from tests import affine_cases as ac
from tests import dct_oracle as do
from tests.helpers import assert_fused_close, bb_to_dicts, run_both, sim_to_view

pytestmark = pytest.mark.gpu

U16, U8, F32 = np.uint16, np.uint8, np.float32
WA, MAX, AVG = "weighted_average", "max", "simple_average"
COUNTERS = ("fuse_rows_chunks", "fuse_region_chunks", "fuse_column_chunks", "fuse_generic_chunks")


def _cells():
    cells = []
    for name in ("fan3d_12", "fan2d_12"):
        cells += [(name, dtype, order, WA) for dtype in (U16, U8, F32) for order in (0, 1)]
    cells += [("fan2d_70", dtype, 1, WA) for dtype in (U16, F32)]
    for name in ("knife_rot90_2d", "knife_rot90_3d"):
        cells += [(name, dtype, order, fusion) for fusion in (MAX, AVG) for dtype in (U16, F32) for order in (0, 1)]
        cells.append((name, F32, 1, WA))
    cells += [("mirror_swap", dtype, order, fusion) for fusion in (WA, MAX, AVG) for dtype in (U8, F32) for order in (0, 1)]
    for name in ("shear_aniso", "trimmed", "far_origin"):
        cells += [(name, dtype, 1, fusion) for fusion in (WA, MAX) for dtype in (U16, F32)]
    cells += [("trimmed", dtype, 0, fusion) for fusion in (WA, MAX) for dtype in (U16, F32)]
    return cells


def _cell_id(cell):
    name, dtype, order, fusion = cell
    return f"{name}-{np.dtype(dtype).name}-order{order}-{fusion}"


def _reset_counters():
    from multiview_stitcher_amd import _lib

    for key in COUNTERS:
        _lib.get_counter(key, reset=True)


def _assert_went_generic(at_least=1):
    """The chunk counters since ``_reset_counters``: the generic kernel fused, no other family did."""
    from multiview_stitcher_amd import _lib

    seen = {key: _lib.get_counter(key) for key in COUNTERS}
    assert seen["fuse_generic_chunks"] >= at_least, seen
    assert seen["fuse_rows_chunks"] == seen["fuse_region_chunks"] == seen["fuse_column_chunks"] == 0, seen


@pytest.mark.parametrize("cell", _cells(), ids=_cell_id)
def test_generic_kernel_matches_oracle(hip_device, cell):
    name, dtype, order, fusion = cell
    sims, params, out_bb, kw = ac.build(name, dtype)
    _reset_counters()
    got, want, want_f = run_both(list(sims), list(params), out_bb, fusion=fusion, interpolation_order=order, **kw)
    _assert_went_generic()
    assert got.shape == tuple(int(n) - 2 * kw.get("trim_overlap_in_pixels", 0) for n in out_bb["shape"])
    stats = assert_fused_close(got, want, want_f[0], noise_floor=want_f[1])
    print(f"{_cell_id(cell)}: {stats}")
    if dtype == F32:
        assert np.isfinite(got).all(), stats
    if name.startswith("knife") and dtype == F32 and fusion in (MAX, AVG):
        # strictly positive tiles: a voxel is 0 exactly where no view is in bounds -- the classification, voxel for voxel
        mism = int(((got == 0) != (want == 0)).sum())
        assert np.array_equal(got == 0, want == 0), f"{mism} voxels classified unlike the oracle; {stats}"
    assert float((got != 0).mean()) >= 0.3, stats


def test_one_rotated_view_sends_the_whole_chunk_to_the_generic_kernel(hip_device):
    """Three views under integer translations (identity pixel matrices) and one turned by 30 degrees: no kernel family but the generic
    one handles that view, and a chunk is fused by one family."""
    sims, params, out_bb, kw = ac.build("mirror_swap_one_rotated", U16)
    _reset_counters()
    got, want, want_f = run_both(list(sims), list(params), out_bb, **kw)
    _assert_went_generic()
    stats = assert_fused_close(got, want, want_f[0], noise_floor=want_f[1])
    print(f"mirror_swap_one_rotated: {stats}")


@pytest.mark.parametrize("name,dtype", [("fan2d_12", F32), ("fan2d_12", U16), ("shear_aniso", F32), ("shear_aniso", U16)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_dct_weights_through_the_generic_kernel(hip_device, name, dtype):
    """fuse_kernel<..., DCT = true> with more than 8 views on a brick and with sheared 3D views: fuse_np with the GPU's DCT-entropy
    weights against fuse_np with the numpy / scipy restatement as a host callable, at the bar of
    tests/test_dct_weights_gpu.py::test_fuse_np_matches_oracle_callable."""
    from multiview_stitcher_amd import fusion

    sims, params, out_bb, kw = ac.build(name, dtype)
    sims, params = list(sims), list(params)
    ndim = len(out_bb["shape"])
    sd = ["z", "y", "x"][-ndim:]
    fvb = [bb_to_dicts(sim_to_view(s)[1], sd) for s in sims]
    wkw = {"dct_size": 8} if ndim == 3 else {"dct_size": 16, "otf_support_fraction": 0.25}
    _reset_counters()
    got = fusion.fuse_np(sims, params, bb_to_dicts(out_bb, sd), full_view_bbs=fvb, weights_func=fusion.content_based_dct,
                         weights_func_kwargs=wkw, **kw)
    _assert_went_generic()
    want = fusion.fuse_np(sims, params, bb_to_dicts(out_bb, sd), full_view_bbs=fvb, weights_func=do.content_based_dct,
                          weights_func_kwargs=wkw, **kw)
    assert got.dtype == np.dtype(dtype) and got.shape == want.shape
    assert np.abs(got.astype(np.float64)).max() > 0
    if dtype == F32:
        assert_fused_close(got, want)
    else:
        assert np.abs(got.astype(np.int64) - want.astype(np.int64)).max() <= 1


@pytest.mark.parametrize("dtype", [U16, U8, F32], ids=lambda v: np.dtype(v).name)
def test_chunked_fuse_equals_the_single_chunk(hip_device, dtype):
    """fusion.fuse() of fan3d_12's views in 2 x 2 chunks along y and x, every chunk with its own slabs, against the single-chunk
    fuse_np of the same views: a voxel sees the same views in the same order (the cull keeps view order), so every dtype is equal bit
    for bit."""
    from multiview_stitcher_amd import fusion, spatial_image_utils as si

    sims, params, out_bb, _ = ac.build("fan3d_12", dtype)
    sd = ["z", "y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    full = []
    for v, p in zip(views, params):
        full.append(si.get_sim_from_array(v["data"], dims=sd, scale=dict(zip(sd, v["spacing"].tolist())),
                                          translation=dict(zip(sd, v["origin"].tolist())), affine=p, transform_key="k"))
    props = bb_to_dicts(out_bb, sd)
    shape = [int(n) for n in out_bb["shape"]]
    chunks = {"z": shape[0], "y": (shape[1] + 1) // 2, "x": (shape[2] + 1) // 2}
    _reset_counters()
    fused = fusion.fuse(full, transform_key="k", output_stack_properties=props, output_chunksize=chunks, merge_chunks=False)
    _assert_went_generic(at_least=4)
    _reset_counters()
    single = fusion.fuse_np(list(sims), list(params), props, full_view_bbs=[bb_to_dicts(b, sd) for b in bbs])
    _assert_went_generic()
    got = np.asarray(fused.data).reshape(single.shape)
    assert got.dtype == single.dtype and float((single != 0).mean()) > 0.3
    differ = got != single
    worst = float(np.abs(got.astype(np.float64) - single.astype(np.float64)).max())
    assert np.array_equal(got, single), f"{int(differ.sum())} of {differ.size} voxels differ, by {worst:.3e} at most"
