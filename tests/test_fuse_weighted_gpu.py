"""GPU: ``fusion.fuse_np(..., view_weights=)`` / ``fusion.fuse(..., view_weights=)`` (mvs_fuse_chunk_weighted,
csrc/mvs_fuse_weighted.hip) against tests/mask_fuse_oracle.py.

The views are the cases of tests/affine_cases.py with real matrices -- 12 views turned about a centre (fan2d_12: 2-D bricks, more
than 8 views on a brick), shear with anisotropic spacings and a negative determinant (shear_aniso, and trimmed: a result width
that is no multiple of 4), turns by exactly pi / 2 on a grid where every third output voxel has a coordinate an integer -+ k 1e-10
(knife_rot90_3d: what decides whether a tile edge takes part) -- and the weight tiles ``masks.feather`` of smooth random blob masks.
Every case checks shape and dtype, that at least 30 % of the voxels are nonzero, and that at at least 5 % of the voxels some view has
0 < m < 1 while another view takes part: otherwise it would show nothing about the feather.

Parity is ``helpers.assert_fused_close`` at its defaults: float32 within 1e-4 relative, integers within one count and only next to an
integer boundary of the reference's float result, the reference's own noise floor on at most 1 % of the voxels."""
import functools

import numpy as np
import pytest

from tests import affine_cases as ac
from tests import fuse_weight_cases as wc
from tests import mask_feather_oracle as feather_oracle
from tests import mask_fuse_oracle as mfo
from tests.helpers import assert_fused_close, bb_to_dicts, placed_tiles, reference_noise_floor, same_bits, sim_to_view

pytestmark = pytest.mark.gpu

U16, U8, F32 = np.uint16, np.uint8, np.float32
WA, MAX, AVG = "weighted_average", "max", "simple_average"
COUNTERS = ("fuse_rows_chunks", "fuse_region_chunks", "fuse_column_chunks", "fuse_generic_chunks", "fuse_weighted_chunks")


def _funcs():
    from multiview_stitcher_amd import fusion

    return {WA: fusion.weighted_average_fusion, MAX: fusion.max_fusion, AVG: fusion.simple_average_fusion}


def _reset_counters():
    from multiview_stitcher_amd import _lib

    for key in COUNTERS:
        _lib.get_counter(key, reset=True)


def _assert_went_weighted(at_least=1):
    """The chunk counters since ``_reset_counters``: the weighted kernel fused, no family of mvs_fuse_chunk did."""
    from multiview_stitcher_amd import _lib

    counts = {key: int(_lib.get_counter(key)) for key in COUNTERS}
    assert counts["fuse_weighted_chunks"] >= at_least and sum(counts.values()) == counts["fuse_weighted_chunks"], counts


@functools.lru_cache(maxsize=None)
def _gpu_tiles(name, dtype, device):
    """The weight tiles of a case from ``masks.feather`` on the device; they are the oracle's (the precondition of
    tests/test_mask_feather_gpu.py asserted first).  Built once per case; leave them unchanged."""
    from multiview_stitcher_amd import masks

    tiles = []
    for mask, want in zip(wc.masks_of(name, dtype), wc.feathered_tiles(name, dtype)):
        width = wc.WIDTHS[mask.ndim]
        assert feather_oracle.half_integer_distance(feather_oracle.feather_float(mask, width)) > 1e-9
        got = masks.feather(np.array(mask), width, device=device)
        assert np.array_equal(got, want)
        tiles.append(got)
    return tuple(tiles)


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype, fusion_name, order):
    sims, params, out_bb, kw = ac.build(name, dtype)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    tiles = [dict(v, data=t) for v, t in zip(views, wc.feathered_tiles(name, dtype))]
    return mfo.fuse_np(list(views), list(params), out_bb, tiles, fusion=fusion_name, interpolation_order=order, full_view_bbs=list(bbs), **kw)


def _check_says_something(got, want, dbg, min_feather=0.05):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert float((got != 0).mean()) >= 0.3
    sl = (slice(None),) + tuple(slice(t, -t) if t > 0 else slice(None) for t in dbg["trim"])
    assert wc.feather_shows(dbg["m"][sl], dbg["views"][sl]) >= min_feather


def _fuse_np(name, dtype, fusion_name, order, view_weights, device):
    from multiview_stitcher_amd import fusion

    sims, params, out_bb, kw = ac.build(name, dtype)
    sd = ["z", "y", "x"][-len(out_bb["shape"]):]
    bbs = [sim_to_view(s)[1] for s in sims]
    return fusion.fuse_np(list(sims), list(params), bb_to_dicts(out_bb, sd), fusion_func=_funcs()[fusion_name], interpolation_order=order,
                          full_view_bbs=[bb_to_dicts(b, sd) for b in bbs], trim_overlap_in_pixels=kw.get("trim_overlap_in_pixels", 0),
                          view_weights=view_weights, device=device)


def _cells():
    cells = [(name, dtype, order, fusion_name) for name in ("fan2d_12", "shear_aniso", "knife_rot90_3d") for dtype in (U16, U8, F32)
             for order in (0, 1) for fusion_name in (WA, MAX, AVG)]
    cells += [("trimmed", U16, order, fusion_name) for order in (0, 1) for fusion_name in (WA, MAX, AVG)]
    return cells


@pytest.mark.parametrize("cell", _cells(), ids=lambda c: f"{c[0]}-{np.dtype(c[1]).name}-order{c[2]}-{c[3]}")
def test_parity_with_the_oracle(cell, hip_device):
    name, dtype, order, fusion_name = cell
    sims = ac.build(name, dtype)[0]
    tiles = [wc.tile_sim(t, s) for t, s in zip(_gpu_tiles(name, np.dtype(dtype), hip_device), sims)]
    want, want_f, dbg = _oracle(name, np.dtype(dtype), fusion_name, order)
    _reset_counters()
    got = _fuse_np(name, dtype, fusion_name, order, tiles, hip_device)
    _assert_went_weighted()
    _check_says_something(got, want, dbg)
    assert_fused_close(got, want, want_f, noise_floor=reference_noise_floor(dbg, want_f))
    if fusion_name != WA:
        assert np.array_equal(got == 0, want == 0)      # which views take part decides the value by whole counts: the zero mask is exact


@pytest.mark.parametrize("dtype", [U16, F32], ids=lambda v: np.dtype(v).name)
def test_binned_weight_tile(dtype, hip_device):
    """The weight tiles on a grid binned by 2 with the binned origin (what ``sample_masks(binning=2)`` returns), through sims: the
    tile's own coordinates are used, and where the coarse grid ends half a block inside the image the clamp keeps the rim."""
    from multiview_stitcher_amd import masks, spatial_image_utils as si

    name = "fan2d_12"
    sims, params, out_bb, kw = ac.build(name, dtype)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    tiles, otiles = [], []
    for i, (s, v) in enumerate(zip(sims, views)):
        shape = tuple(n // 2 for n in v["data"].shape)
        mask = wc.fc.blob_mask(shape, seed=300 + i, sigma=2.0)
        assert feather_oracle.half_integer_distance(feather_oracle.feather_float(mask, (3, 5))) > 1e-9
        w = masks.feather(np.array(mask), (3, 5), device=hip_device)
        origin = {d: float(o + 0.5 * sp) for d, o, sp in zip(("y", "x"), v["origin"], v["spacing"])}      # the mean of every pair of coordinates
        spacing = {d: float(2 * sp) for d, sp in zip(("y", "x"), v["spacing"])}
        tiles.append(wc.tile_sim(w, s, origin, spacing))
        otiles.append({"data": w, "origin": np.array([origin["y"], origin["x"]]), "spacing": np.array([spacing["y"], spacing["x"]])})
        assert np.array_equal(si.get_spacing_from_sim(tiles[-1], asarray=True), otiles[-1]["spacing"])
    want, want_f, dbg = mfo.fuse_np(list(views), list(params), out_bb, otiles, full_view_bbs=list(bbs), **kw)
    got = _fuse_np(name, dtype, WA, 1, tiles, hip_device)
    _check_says_something(got, want, dbg)
    assert_fused_close(got, want, want_f, noise_floor=reference_noise_floor(dbg, want_f))


@pytest.mark.parametrize("fusion_name", [WA, MAX, AVG])
def test_mixed_weights_none_and_all_zero(fusion_name, hip_device):
    """shear_aniso with a feathered tile on view 0, no tile on view 1 and an all-zero tile on view 2 (the view disappears)."""
    name, dtype = "shear_aniso", U16
    sims, params, out_bb, kw = ac.build(name, dtype)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    t0 = _gpu_tiles(name, np.dtype(dtype), hip_device)[0]
    zero = np.zeros(views[2]["data"].shape, np.uint8)
    otiles = [dict(views[0], data=t0), None, dict(views[2], data=zero)]
    want, want_f, dbg = mfo.fuse_np(list(views), list(params), out_bb, otiles, fusion=fusion_name, full_view_bbs=list(bbs), **kw)
    got = _fuse_np(name, dtype, fusion_name, 1, [wc.tile_sim(t0, sims[0]), None, zero], hip_device)      # (a plain array takes the view's grid)
    _check_says_something(got, want, dbg)
    assert np.isnan(dbg["views"][2]).all() and (~np.isnan(ac.oracle(name, dtype, fusion_name, 1)[2]["views"][2])).sum() > 0      # (it did reach the chunk)
    assert_fused_close(got, want, want_f, noise_floor=reference_noise_floor(dbg, want_f))
    if fusion_name != WA:
        assert np.array_equal(got == 0, want == 0)


@pytest.mark.parametrize("name", ["fan2d_12", "shear_aniso", "trimmed"])
@pytest.mark.parametrize("fusion_name", [WA, MAX, AVG])
@pytest.mark.parametrize("dtype", [U16, U8, F32], ids=lambda v: np.dtype(v).name)
def test_full_weights_equal_the_plain_fuse_bit_for_bit(dtype, fusion_name, name, hip_device):
    """All-252 tiles give m == 1 exactly, and the weighted kernel then performs the generic kernel's float32 operations in its order:
    the result has the bits of ``fuse_np`` without weights (these views send the plain call to the generic kernel), for every dtype
    and fusion function, at order 0 and 1."""
    from multiview_stitcher_amd import _lib

    sims = ac.build(name, dtype)[0]
    full = [np.full(s.data.shape, 252, np.uint8) for s in sims]
    for order in (0, 1):
        _reset_counters()
        plain = _fuse_np(name, dtype, fusion_name, order, None, hip_device)
        assert int(_lib.get_counter("fuse_generic_chunks")) == 1 and int(_lib.get_counter("fuse_weighted_chunks")) == 0
        got = _fuse_np(name, dtype, fusion_name, order, full, hip_device)
        assert float((got != 0).mean()) >= 0.3
        assert same_bits(got, plain), f"{int((got != plain).sum())} of {got.size} voxels differ"
        over = _fuse_np(name, dtype, fusion_name, order, [np.full(s.data.shape, 255, np.uint8) for s in sims], hip_device)
        assert same_bits(over, plain)                  # a stored value above 252 counts as 252


@pytest.mark.parametrize("dtype", [U16, U8, F32], ids=lambda v: np.dtype(v).name)
def test_chunked_fuse_equals_the_single_chunk(hip_device, dtype):
    """fusion.fuse() of fan3d_12's views and tiles in 2 x 2 chunks along y and x against the single-chunk fuse_np: a voxel sees the
    same views in the same order (the cull keeps view order), so every dtype is equal bit for bit; resident and host tiles alike."""
    from multiview_stitcher_amd import fusion, spatial_image_utils as si
    from multiview_stitcher_amd.device import DeviceArray

    name = "fan3d_12"
    sims, params, out_bb, _ = ac.build(name, dtype)
    sd = ["z", "y", "x"]
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    full = [si.get_sim_from_array(v["data"], dims=sd, scale=dict(zip(sd, v["spacing"].tolist())), translation=dict(zip(sd, v["origin"].tolist())),
                                  affine=p, transform_key="k") for v, p in zip(views, params)]
    tiles = [wc.tile_sim(t, s) for t, s in zip(_gpu_tiles(name, np.dtype(dtype), hip_device), sims)]
    given = [t if i % 2 else t.copy(data=DeviceArray.from_host(np.asarray(t.data), hip_device)) for i, t in enumerate(tiles)]
    props = bb_to_dicts(out_bb, sd)
    shape = [int(n) for n in out_bb["shape"]]
    chunks = {"z": shape[0], "y": (shape[1] + 1) // 2, "x": (shape[2] + 1) // 2}
    _reset_counters()
    fused = fusion.fuse(full, transform_key="k", output_stack_properties=props, output_chunksize=chunks, merge_chunks=False, view_weights=given,
                        device=hip_device)
    _assert_went_weighted(at_least=4)
    _reset_counters()
    single = fusion.fuse_np(list(sims), list(params), props, full_view_bbs=[bb_to_dicts(b, sd) for b in bbs], view_weights=tiles, device=hip_device)
    _assert_went_weighted()
    want, want_f, dbg = _oracle(name, np.dtype(dtype), WA, 1)
    _check_says_something(single, want, dbg)
    assert_fused_close(single, want, want_f, noise_floor=reference_noise_floor(dbg, want_f))
    got = np.asarray(fused.data).reshape(single.shape)
    differ = got != single
    worst = float(np.abs(got.astype(np.float64) - single.astype(np.float64)).max())
    assert np.array_equal(got, single), f"{int(differ.sum())} of {differ.size} voxels differ, by {worst:.3e} at most"
    on_device = fusion.fuse(full, transform_key="k", output_stack_properties=props, view_weights=given, output_on_backend=True, device=hip_device)
    assert same_bits(on_device.data.get().reshape(single.shape), single)      # one merged launch block, the result left on the device


def test_end_to_end_sample_masks_feather_fuse(hip_device):
    """sample_masks -> feather -> fuse(view_weights=) on a 2 x 2 mosaic of white-noise tiles: one tile's corner inside the overlap is
    zeroed (a shadow), the sample mask finds it, and in the overlap the dark corner no longer pulls the result down."""
    from multiview_stitcher_amd import fusion, masks, spatial_image_utils as si

    shape, origins = (48, 64), [(0, 0), (0, 40), (28, 0), (28, 40)]
    sims = placed_tiles(U16, shape, origins, seed=5)
    for s in sims:
        s.data[...] = s.data // 2 + 20000                    # bright everywhere: the threshold separates the shadow alone
        si.set_sim_affine(s, np.eye(3), "k")
    sims[0].data[22:, 36:] = 0                               # tile 0's corner: the overlaps with tiles 1, 2 and 3 and a little more
    mask_sims = masks.sample_masks(sims, threshold=1000.0, device=hip_device)
    assert mask_sims[0].data[22:, 36:].max() == 0 and all(int(m.data.min()) == 1 for m in mask_sims[1:])
    tiles = [masks.feather(m, (12, 12), device=hip_device) for m in mask_sims]
    assert tiles[0].data[22:, 36:].max() == 0 and tiles[0].data[:10, :20].min() == 252 and np.all(tiles[1].data == 252)
    plain = np.asarray(fusion.fuse(sims, transform_key="k", device=hip_device).data)
    fused = fusion.fuse(sims, transform_key="k", view_weights=tiles, device=hip_device)
    got = np.asarray(fused.data)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    out_bb = {"origin": np.array([np.asarray(fused.coords[d])[0] for d in ("y", "x")], dtype=np.float64), "spacing": np.ones(2),
              "shape": np.array(got.shape)}
    assert got.shape == (76, 104) and np.all(out_bb["origin"] == 0)
    otiles = [dict(v, data=np.asarray(t.data)) for v, t in zip(views, tiles)]
    want, want_f, dbg = mfo.fuse_np(list(views), [np.eye(3)] * 4, out_bb, otiles, full_view_bbs=list(bbs))
    _check_says_something(got, want, dbg)
    assert_fused_close(got, want, want_f, noise_floor=reference_noise_floor(dbg, want_f))
    corner = (slice(30, 46), slice(42, 62))                  # inside the shadow and inside tiles 1, 2 and 3
    assert got[corner].min() >= 20000 and plain[corner].min() < 20000 and float(plain[corner].mean()) < float(got[corner].mean()) - 1000
    far = (slice(0, 10), slice(0, 20))
    assert np.array_equal(got[far], plain[far])              # one view, full weight: untouched
