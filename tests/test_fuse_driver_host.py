"""fusion.fuse's host driver without a GPU: ``fusion.fuse_np`` is replaced by a recording stand-in that returns every block
filled with the index of its call, so what is checked is what the driver DECIDES -- which blocks exist, which views and index
windows feed each, where each lands, what ends up in a store.  The expectations are independent statements: the views and
windows come from the restatement of the reference's planner (oracle/plan_oracle.py), a block's place in the result from its
box's offset in the output stack, the store's chunk grid from the request."""
import os

import numpy as np
import pytest

from multiview_stitcher_amd import fusion, msi_utils, mv_graph, ngff_utils, zarr_io
from multiview_stitcher_amd import spatial_image_utils as si
from oracle import plan_oracle as po

KEY = "k"


class StandIn:
    """fuse_np: records the keyword arguments, returns the block (box minus trimmed halo) filled with the call's number."""

    def __init__(self):
        self.calls = []

    def __call__(self, **kw):
        box, trim = kw["output_properties"], kw["trim_overlap_in_pixels"]
        shape = tuple(int(box["shape"][d]) - 2 * int(trim[d] if isinstance(trim, dict) else trim) for d in box["shape"])
        self.calls.append(kw)
        return np.full(shape, len(self.calls), dtype=kw["sims"][0].dtype)


@pytest.fixture
def stand_in(monkeypatch):
    rec = StandIn()
    monkeypatch.setattr(fusion, "fuse_np", rec)
    return rec


def _mosaic(ndim, ns_shape=(), t_shift=None, spacing=None, tile=None, frac=False):
    """2 x 2 (x 1 in z) tiles.  Voxels of view ``iv`` in field ``f`` (C order over ``ns_shape``) hold ``100 * f + iv + 1``, so a slab
    tells which view and field it was cut from.  ``t_shift``: x translation of view 1 per time point (a t-stacked affine)."""
    sdims = ["z", "y", "x"][-ndim:]
    tile = tile or (12, 40, 48)[-ndim:]
    spacing = spacing or (2.0, 1.0, 1.0)[-ndim:]
    views = []
    for iv, idx in enumerate(np.ndindex(*((1,) * (ndim - 2) + (2, 2)))):
        data = np.empty(tuple(ns_shape) + tuple(tile), np.uint16)
        for f, ns in enumerate(np.ndindex(*ns_shape) if ns_shape else [()]):
            data[ns] = 100 * f + iv + 1
        origin = {d: i * int(n * 0.8) * sp for d, i, n, sp in zip(sdims, idx, tile, spacing)}
        affine = np.eye(ndim + 1)
        if iv == 3:
            shift = (0.0, 0.5, -1.25) if frac else (0.0, -1.0, 2.0)      # (in pixels; z stays on the grid)
            affine[:ndim, ndim] = np.asarray(shift[-ndim:]) * spacing
        if iv == 1 and t_shift is not None:
            affine = np.stack([affine] * len(t_shift))
            affine[:, ndim - 1, ndim] = t_shift
        sim = si.to_spatial_image(data, dims=["c", "t"][2 - len(ns_shape):] + sdims, scale=dict(zip(sdims, spacing)), translation=origin)
        si.set_sim_affine(sim, affine, KEY)
        views.append(sim)
    return views, sdims


def _stack(views, sdims):
    """Output stack of the test's own making: the union of the views' translated boxes at the views' spacing."""
    lo, hi = [], []
    sp = si.get_spacing_from_sim(views[0])
    for v in views:
        p = np.asarray(si.get_affine_from_sim(v, KEY))
        for p_t in (p if p.ndim == 3 else [p]):
            o = si.get_origin_from_sim(v)
            lo.append([o[d] + p_t[k, -1] for k, d in enumerate(sdims)])
            hi.append([o[d] + (v.sizes[d] - 1) * sp[d] + p_t[k, -1] for k, d in enumerate(sdims)])
    lo, hi = np.min(lo, 0), np.max(hi, 0)
    return {"origin": dict(zip(sdims, lo.tolist())), "spacing": dict(sp),
            "shape": {d: int(np.floor((h - l) / sp[d] + 1e-9)) + 1 for d, l, h in zip(sdims, lo, hi)}}


def _expected_blocks(views, sdims, osp, chunks, halo, order, it=0):
    """The blocks of the chunk grid ``chunks`` as the reference's planner (restated in oracle/plan_oracle.py) feeds them: per block its
    grid index, its box with the halo, its offset in the output stack, and [(view, lo, n)] as the label selection picks them."""
    views_bb = [si.get_stack_properties_from_sim(v) for v in views]
    sparams = [np.asarray(p)[it] if np.asarray(p).ndim == 3 else np.asarray(p) for p in (si.get_affine_from_sim(v, KEY) for v in views)]
    cbb, bidx = mv_graph.get_chunk_bbs(osp, chunks)
    cbb_ov = [cb | {"origin": {d: cb["origin"][d] - halo[d] * osp["spacing"][d] for d in sdims}}
              | {"shape": {d: cb["shape"][d] + 2 * halo[d] for d in sdims}} for cb in cbb]
    plan = po._build_spatial_fusion_plan(
        sparams=sparams, views_bb=views_bb, output_stack_properties=osp, output_chunksize=chunks, output_chunk_bbs=cbb,
        output_chunk_bbs_with_overlap=cbb_ov, output_chunk_bbs_for_result=cbb, block_indices=bidx, overlap_in_pixels=halo,
        trim_overlap=True, interpolation_order=order, sdims=sdims)
    coords = [{d: np.asarray(v.coords[d]) for d in sdims} for v in views]
    blocks = []
    for e in plan["per_chunk_entries"]:
        offset = [int(round((e["output_bb"]["origin"][d] - osp["origin"][d]) / osp["spacing"][d])) for d in sdims]
        blocks.append({"index": tuple(e["block_index"]), "box": e["output_bb_overlap"], "offset": offset,
                       "shape": [int(e["output_bb"]["shape"][d]) for d in sdims], "planewise": e["fuse_planewise"],
                       "views": [(iv,) + po.slab_windows(coords[iv], obb, sdims) for iv, obb in e["views"]],
                       "params": sparams, "views_bb": views_bb})
    return blocks


def _check_call(call, block, views, sdims, field=0):
    """One recorded fuse_np call against the block the planner expects: box, slabs (view, field, index window), parameters, boxes."""
    pdims = sdims[1:] if block["planewise"] else sdims      # a plane-wise block is a 2D chunk: z is dropped everywhere
    proj = (lambda bb: {k: {d: v[d] for d in pdims} for k, v in bb.items()})
    box = call["output_properties"]
    assert list(box["shape"]) == pdims
    for k in ("origin", "spacing", "shape"):
        assert {d: float(box[k][d]) for d in pdims} == {d: float(block["box"][k][d]) for d in pdims}, (block["index"], k)
    assert len(call["sims"]) == len(block["views"]) == len(call["params"]) == len(call["full_view_bbs"])
    for slab, param, fvb, (iv, lo, n) in zip(call["sims"], call["params"], call["full_view_bbs"], block["views"]):
        assert list(slab.dims) == pdims
        data = np.asarray(slab.data)
        assert data.min() == data.max() == 100 * field + iv + 1, (block["index"], iv)
        got_lo = [int(round((slab.coords[d][0] - views[iv].coords[d][0]) / block["views_bb"][iv]["spacing"][d])) for d in pdims]
        k0 = len(sdims) - len(pdims)
        assert (got_lo, list(data.shape)) == (list(lo[k0:]), list(n[k0:])), (block["index"], iv)
        for d in pdims:      # the slab's coordinates are the view's own in that window
            np.testing.assert_array_equal(slab.coords[d], views[iv].coords[d][lo[sdims.index(d)]:lo[sdims.index(d)] + n[sdims.index(d)]])
        np.testing.assert_array_equal(param, block["params"][iv][k0:, k0:])
        assert proj(fvb) == proj(block["views_bb"][iv]) and list(fvb["shape"]) == pdims


def _drive(stand_in, views, sdims, chunks, *, halo=0, order=1, grid=None, blocks_pass=None, untrimmed=False, **kw):
    """fuse() under the stand-in; checks every call against the planner's blocks of ``grid`` (default: ``chunks``) and returns
    (result image, the assembly the calls imply).  ``blocks_pass``: the test's own statement of which blocks are fused."""
    osp = kw.pop("osp", None) or _stack(views, sdims)
    halo = {d: halo for d in sdims} if not isinstance(halo, dict) else halo
    del stand_in.calls[:]
    res = fusion.fuse(views, transform_key=KEY, output_stack_properties=osp, output_chunksize=chunks, interpolation_order=order,
                      overlap_in_pixels=halo, trim_overlap=not untrimmed, **kw)
    grid = grid(stand_in.calls) if callable(grid) else (grid or chunks)
    ns_dims = [d for d in views[0].dims if d not in sdims]
    ns_shape = tuple(views[0].sizes[d] for d in ns_dims)
    nblocks = [-(-osp["shape"][d] // grid[d]) for d in sdims]
    grown = [2 * halo[d] * nb if untrimmed else 0 for d, nb in zip(sdims, nblocks)]
    want = np.zeros(ns_shape + tuple(osp["shape"][d] + g for d, g in zip(sdims, grown)), np.uint16)
    covered = np.zeros(want.shape[len(ns_shape):], np.int32)
    calls = iter(enumerate(stand_in.calls, start=1))
    for f, ns in enumerate(np.ndindex(*ns_shape) if ns_shape else [()]):
        it = ns[ns_dims.index("t")] if "t" in ns_dims else 0
        for block in _expected_blocks(views, sdims, osp, grid, halo, order, it):
            # where the block lies in the result: its offset in the stack; untrimmed blocks keep their halo and sit side by side
            lo = [o + (2 * halo[d] * bi if untrimmed else 0) for o, d, bi in zip(block["offset"], sdims, block["index"])]
            hi = [l + n + (2 * halo[d] if untrimmed else 0) for l, n, d in zip(lo, block["shape"], sdims)]
            window = tuple(slice(l, h) for l, h in zip(lo, hi))
            if f == 0:
                covered[window] += 1
            if not block["views"] or (blocks_pass is not None and not blocks_pass(block["index"])):
                continue      # no call: the window stays 0
            number, call = next(calls)
            _check_call(call, block, views, sdims, f)
            assert call["trim_overlap_in_pixels"] == (0 if untrimmed else halo)
            assert call["interpolation_order"] == order and call["shrink_distance"] == 0 and call["backend"] == "hip"
            want[tuple(ns) + window] = number
    assert next(calls, None) is None, "more fuse_np calls than blocks with views"
    assert np.all(covered == 1), "the blocks' windows tile the result exactly once"
    return res, want, osp


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("frac", [False, True])
def test_requested_grid_plan_and_tiling(stand_in, ndim, frac):
    """merge_chunks=False: one call per chunk with views, fed as the planner says, landing at its box's offset; chunks without
    views produce no call and stay 0."""
    views, sdims = _mosaic(ndim, frac=frac)
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    osp = _stack(views, sdims)
    osp["origin"] = {d: osp["origin"][d] - 30 * osp["spacing"][d] for d in sdims}      # a margin: chunks that no view reaches
    osp["shape"] = {d: osp["shape"][d] + 45 for d in sdims}
    for order in (0, 1):
        res, want, _ = _drive(stand_in, views, sdims, chunks, order=order, merge_chunks=False, osp=osp)
        np.testing.assert_array_equal(np.asarray(res.data), want)
        assert (want == 0).any() and len(stand_in.calls) > 8
        assert list(res.dims) == sdims and si.get_origin_from_sim(res) == osp["origin"] and si.get_spacing_from_sim(res) == osp["spacing"]
        np.testing.assert_array_equal(si.get_affine_from_sim(res, KEY), np.eye(ndim + 1))


def _observed_grid(sdims, osp):
    """The launch-block size read from the first recorded call; it must be made of whole requested chunks (or reach the stack's end)."""
    return lambda calls: {d: int(calls[0]["output_properties"]["shape"][d]) for d in sdims}


@pytest.mark.parametrize("ndim", [2, 3])
def test_merged_launch_blocks_tile_the_stack(stand_in, ndim, monkeypatch):
    """merge_chunks (default): one block when the stack fits the budget; with a small MAX_LAUNCH_BYTES several blocks of whole
    requested chunks, each within the budget, fed as the planner feeds a grid of that block size, tiling the result once."""
    views, sdims = _mosaic(ndim)
    chunks = dict(zip(sdims, (4, 16, 16)[-ndim:]))
    osp = _stack(views, sdims)
    res, want, _ = _drive(stand_in, views, sdims, chunks, grid=_observed_grid(sdims, osp))
    assert len(stand_in.calls) == 1 and np.all(want == 1)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    budget = 6000 if ndim == 2 else 40_000
    monkeypatch.setattr(fusion, "MAX_LAUNCH_BYTES", budget)
    res, want, _ = _drive(stand_in, views, sdims, chunks, grid=_observed_grid(sdims, osp))
    np.testing.assert_array_equal(np.asarray(res.data), want)
    assert len(stand_in.calls) > 1
    for call in stand_in.calls:
        shape = call["output_properties"]["shape"]
        assert int(np.prod(list(shape.values()))) * 2 <= budget
    first = stand_in.calls[0]["output_properties"]["shape"]
    assert all(first[d] % chunks[d] == 0 or first[d] == osp["shape"][d] for d in sdims)


@pytest.mark.parametrize("ndim", [2, 3])
def test_halo_trimmed_and_untrimmed(stand_in, ndim):
    """overlap_in_pixels: blocks are fused with the halo.  Trimmed, the result is the stack; with trim_overlap=False it is larger by
    twice the halo per chunk and axis and every untrimmed block sits in its own window."""
    views, sdims = _mosaic(ndim)
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    halo = dict(zip(sdims, (1, 2, 3)[-ndim:]))
    res, want, osp = _drive(stand_in, views, sdims, chunks, halo=halo)
    assert tuple(res.shape) == tuple(osp["shape"][d] for d in sdims)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    n_trimmed = len(stand_in.calls)
    res, want, osp = _drive(stand_in, views, sdims, chunks, halo=halo, untrimmed=True)
    assert tuple(res.shape) == tuple(osp["shape"][d] + 2 * halo[d] * -(-osp["shape"][d] // chunks[d]) for d in sdims)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    assert len(stand_in.calls) == n_trimmed > 4


def test_content_based_sets_its_own_halo(stand_in):
    """content_based asks for a halo of 2 * sigma_2 (its ``required_overlap``): the blocks are cut with it and it is trimmed."""
    views, sdims = _mosaic(2)
    kw = dict(weights_func=fusion.content_based, weights_func_kwargs={"sigma_1": 1, "sigma_2": 2})
    res, want, _ = _drive(stand_in, views, sdims, {"y": 16, "x": 20}, halo=4, **kw)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    assert all(c["weights_func"] is fusion.content_based and c["weights_func_kwargs"] == kw["weights_func_kwargs"] for c in stand_in.calls)
    with pytest.raises(AssertionError):      # (the same call described with a smaller halo does not match)
        _drive(stand_in, views, sdims, {"y": 16, "x": 20}, halo=3, **kw)


@pytest.mark.parametrize("ndim", [2, 3])
def test_chunk_filter(stand_in, ndim):
    """Only the blocks the filter accepts are fused; rejected windows stay 0."""
    views, sdims = _mosaic(ndim)
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    accept = lambda bi: (sum(bi) % 3) != 1
    res, want, _ = _drive(stand_in, views, sdims, chunks, chunk_filter=accept, blocks_pass=accept)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    n_some = len(stand_in.calls)
    assert (want == 0).any()
    res, want, _ = _drive(stand_in, views, sdims, chunks, merge_chunks=False)
    assert n_some < len(stand_in.calls) and not (want == 0).any()


@pytest.mark.parametrize("ndim", [2, 3])
def test_fields_and_time_dependent_affines(stand_in, ndim):
    """(c, t) fields: every field gets its own calls, cut from that field, and the plan of a time point follows its affines."""
    views, sdims = _mosaic(ndim, ns_shape=(2, 3), t_shift=[0.0, 9.0, 21.0])
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    res, want, osp = _drive(stand_in, views, sdims, chunks, merge_chunks=False)
    assert list(res.dims) == ["c", "t"] + sdims and res.shape[:2] == (2, 3)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    # the plans of the time points differ: the expectations of t = 0 do not describe t = 2
    b0 = _expected_blocks(views, sdims, osp, chunks, {d: 0 for d in sdims}, 1, 0)
    b2 = _expected_blocks(views, sdims, osp, chunks, {d: 0 for d in sdims}, 1, 2)
    assert [b["views"] for b in b0] != [b["views"] for b in b2]
    # merged: one launch block per field
    res, want, _ = _drive(stand_in, views, sdims, chunks, grid=_observed_grid(sdims, osp))
    assert len(stand_in.calls) == 6
    np.testing.assert_array_equal(np.asarray(res.data), want)


@pytest.mark.parametrize("to_zarr", [False, True])
def test_planewise_blocks(stand_in, tmp_path, to_zarr):
    """Chunks one plane thick on the views' z grid are fused as 2D chunks: 2D slabs, 2D parameters, projected boxes; each lands as
    one plane of the 3D result (host array or store)."""
    views, sdims = _mosaic(3, tile=(3, 20, 24))
    chunks = {"z": 1, "y": 16, "x": 16}
    res, want, osp = _drive(stand_in, views, sdims, chunks, **({"output_zarr_url": str(tmp_path / "out.zarr")} if to_zarr else {}))
    assert osp["shape"]["z"] == 3 and res.shape[0] == 3
    np.testing.assert_array_equal(np.asarray(res.data), want)
    assert all(list(s.dims) == ["y", "x"] for c in stand_in.calls for s in c["sims"])
    assert all(np.asarray(p).shape == (3, 3) for c in stand_in.calls for p in c["params"])
    planes = [np.unique(np.asarray(res.data)[z]) for z in range(3)]
    assert not set(planes[0]) & set(planes[1]) and not set(planes[1]) & set(planes[2])


def _custom_fusion(transformed_views, blending_weights):
    return np.nansum(transformed_views * blending_weights, axis=0)


@pytest.mark.parametrize("ndim", [2, 3])
def test_frame_origin(stand_in, ndim):
    """The index frame's origin is the output stack's by default and the caller's when passed; user callables get none."""
    views, sdims = _mosaic(ndim)
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    _, _, osp = _drive(stand_in, views, sdims, chunks, merge_chunks=False)
    assert len(stand_in.calls) > 4 and all(c["frame_origin"] == osp["origin"] for c in stand_in.calls)
    mine = {d: osp["origin"][d] - 7.0 for d in sdims}
    _drive(stand_in, views, sdims, chunks, merge_chunks=False, frame_origin=mine)
    assert all(c["frame_origin"] == mine for c in stand_in.calls)
    _drive(stand_in, views, sdims, chunks, weights_func=fusion.content_based, halo=22)
    assert all(c["frame_origin"] == osp["origin"] for c in stand_in.calls)
    _drive(stand_in, views, sdims, chunks, fusion_func=_custom_fusion)
    assert stand_in.calls and all("frame_origin" not in c and c["fusion_func"] is _custom_fusion for c in stand_in.calls)
    del stand_in.calls[:]
    fusion.fuse(views, transform_key=KEY, output_chunksize=chunks, fusion_func=fusion.multi_view_deconvolution)
    assert stand_in.calls and all("frame_origin" not in c for c in stand_in.calls)


def test_planewise_frame_origin_is_projected(stand_in):
    views, sdims = _mosaic(3, tile=(3, 20, 24))
    _, _, osp = _drive(stand_in, views, sdims, {"z": 1, "y": 16, "x": 16})
    assert all(c["frame_origin"] == {d: osp["origin"][d] for d in ("y", "x")} for c in stand_in.calls)


# ---- Zarr output -----------------------------------------------------------------------------------------------------------

def _store_array(url, ome):
    return zarr_io.ZarrArray.open(os.path.join(url, "0") if ome else url)


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("options", [{}, {"ome_zarr": True}, {"ome_zarr": True, "ngff_version": "0.5"}], ids=["v2", "ome04", "ome05"])
@pytest.mark.parametrize("store_chunks", [None, "spatial", "full"])
def test_zarr_output(stand_in, tmp_path, ndim, options, store_chunks):
    """The store is chunked by the REQUESTED grid (or by ``zarr_array_creation_kwargs["chunks"]``, full-rank or spatial-only), not
    by the merged launch block, and what is read back is what the calls assemble to."""
    views, sdims = _mosaic(ndim, ns_shape=(2, 1))
    chunks = dict(zip(sdims, (4, 16, 16)[-ndim:]))
    url = str(tmp_path / "out.zarr")
    zo = dict(options)
    want_chunks = [chunks[d] for d in sdims]
    if store_chunks:
        want_chunks = [2, 8, 8][-ndim:]
        zo["zarr_array_creation_kwargs"] = {"chunks": ([1, 1] if store_chunks == "full" else []) + want_chunks}
    osp = _stack(views, sdims)
    res, want, _ = _drive(stand_in, views, sdims, chunks, grid=_observed_grid(sdims, osp), output_zarr_url=url, zarr_options=zo)
    assert len(stand_in.calls) == 2      # (merged: one launch block per field)
    arr = _store_array(url, options.get("ome_zarr"))
    assert list(arr.chunks) == [1, 1] + want_chunks and tuple(arr.shape) == want.shape
    np.testing.assert_array_equal(np.asarray(arr[...]), want)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    assert list(res.dims) == ["c", "t"] + sdims
    if options.get("ome_zarr"):
        back = ngff_utils.read_sim_from_ome_zarr(url)
        assert si.get_origin_from_sim(back) == pytest.approx(osp["origin"]) and si.get_spacing_from_sim(back) == pytest.approx(osp["spacing"])
        assert os.path.exists(os.path.join(url, "zarr.json" if options.get("ngff_version") == "0.5" else ".zattrs"))


@pytest.mark.parametrize("ndim", [2, 3])
def test_zarr_inputs(stand_in, tmp_path, ndim):
    """Zarr-backed views: the slabs are windows of the stores, cut as the planner says."""
    host, sdims = _mosaic(ndim)
    views = []
    for i, v in enumerate(host):
        z = ngff_utils.write_sim_to_ome_zarr(v, str(tmp_path / f"in{i}.zarr"))
        assert zarr_io.is_zarr_backed(z.data)
        views.append(z)
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    res, want, _ = _drive(stand_in, views, sdims, chunks, merge_chunks=False)
    np.testing.assert_array_equal(np.asarray(res.data), want)
    assert len(stand_in.calls) > 4


@pytest.mark.parametrize("ndim", [2, 3])
def test_batch_options(stand_in, tmp_path, ndim):
    """batch_func receives batches of n_batch block ids in np.ndindex order over (fields, requested chunk grid); fuse_chunk fuses
    one block and writes its region.  Without a batch_func every block is fused."""
    views, sdims = _mosaic(ndim, ns_shape=(2, 3), t_shift=[0.0, 9.0, 21.0])
    chunks = dict(zip(sdims, (5, 16, 20)[-ndim:]))
    url = str(tmp_path / "out.zarr")
    osp = _stack(views, sdims)
    ids = list(np.ndindex(2, 3, *[-(-osp["shape"][d] // chunks[d]) for d in sdims]))
    batches = []

    def batch_func(func, block_ids, tag):
        assert tag == "x"
        batches.append([tuple(int(i) for i in b) for b in block_ids])
        for b in block_ids:
            assert func(b) is None

    res, want, _ = _drive(stand_in, views, sdims, chunks, output_zarr_url=url,
                          batch_options={"batch_func": batch_func, "n_batch": 7, "batch_func_kwargs": {"tag": "x"}})
    assert batches == [ids[k:k + 7] for k in range(0, len(ids), 7)]
    np.testing.assert_array_equal(np.asarray(_store_array(url, False)[...]), want)
    assert list(_store_array(url, False).chunks) == [1, 1] + [chunks[d] for d in sdims]
    res, want2, _ = _drive(stand_in, views, sdims, chunks, output_zarr_url=url, batch_options={"n_batch": 4})
    np.testing.assert_array_equal(want2, want)
    np.testing.assert_array_equal(np.asarray(res.data), want)


def test_chunk_filter_joins_an_existing_store(stand_in, tmp_path):
    """Farm workers share one store: a call with a chunk_filter neither removes nor recreates what is there, so two calls with
    complementary filters leave the blocks of both."""
    views, sdims = _mosaic(2)
    chunks = {"y": 16, "x": 20}
    url = str(tmp_path / "out.zarr")
    even = lambda bi: sum(bi) % 2 == 0
    odd = lambda bi: not even(bi)
    _, first, _ = _drive(stand_in, views, sdims, chunks, output_zarr_url=url, chunk_filter=even, blocks_pass=even)
    res, second, _ = _drive(stand_in, views, sdims, chunks, output_zarr_url=url, chunk_filter=odd, blocks_pass=odd)
    assert first.any() and second.any() and not (first.astype(bool) & second.astype(bool)).any()
    np.testing.assert_array_equal(np.asarray(_store_array(url, False)[...]), first + second)
    np.testing.assert_array_equal(np.asarray(res.data), first + second)


def test_overwrite_false_joins_an_existing_array(stand_in, tmp_path):
    """zarr_options["overwrite"] = False: an array that exists is opened, not recreated -- it keeps its own chunk grid and the
    voxels no block writes."""
    views, sdims = _mosaic(2)
    chunks = {"y": 16, "x": 16}
    osp = _stack(views, sdims)
    osp["shape"] = {d: n + 40 for d, n in osp["shape"].items()}      # a margin no view reaches: chunks nobody writes
    url = str(tmp_path / "out.zarr")
    shape = [osp["shape"][d] for d in sdims]
    before = zarr_io.ZarrArray.create(url, shape, [8, 8], np.uint16)
    before.write([0, 0], np.full(shape, 7, np.uint16))
    res, want, _ = _drive(stand_in, views, sdims, chunks, output_zarr_url=url, zarr_options={"overwrite": False}, merge_chunks=False, osp=osp)
    arr = _store_array(url, False)
    assert list(arr.chunks) == [8, 8] and (want == 0).any()
    np.testing.assert_array_equal(np.asarray(arr[...]), np.where(want == 0, 7, want))
    # the default removes the store and creates it with the requested grid
    res, want, _ = _drive(stand_in, views, sdims, chunks, output_zarr_url=url, merge_chunks=False, osp=osp)
    arr = _store_array(url, False)
    assert list(arr.chunks) == [16, 16]
    np.testing.assert_array_equal(np.asarray(arr[...]), want)


# ---- multiscale ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [2, 3])
def test_multiscale_inputs(stand_in, ndim):
    """msims in, an msim out: one fuse per level, with the geometry of msi_utils.calc_resolution_levels (centre-of-pixel origins)."""
    sdims = ["z", "y", "x"][-ndim:]
    shape = (6, 230, 250)[-ndim:]
    msims = []
    for iv, x0 in enumerate((0.0, 140.0)):
        sim = si.to_spatial_image(np.full(shape, iv + 1, np.uint16), dims=sdims, scale={d: 1.0 for d in sdims},
                                  translation={d: (x0 if d == "x" else 0.0) for d in sdims})
        si.set_sim_affine(sim, np.eye(ndim + 1), KEY)
        msims.append(msi_utils.get_msim_from_sim(sim, scale_factors=[{d: (1 if d == "z" else 2) for d in sdims}]))
    out = fusion.fuse(msims, transform_key=KEY, output_chunksize={d: 64 for d in sdims})
    assert msi_utils.is_msim(out)
    scale0 = [msi_utils.get_sim_from_msim(m) for m in msims]
    osp0 = fusion.process_output_stack_properties(scale0, transform_key=KEY)
    shapes, _, factors = msi_utils.calc_resolution_levels({d: int(osp0["shape"][d]) for d in sdims})
    keys = msi_utils.get_sorted_scale_keys(out)
    assert len(keys) == len(shapes) == 2 and len(stand_in.calls) == 2
    for key, shp, f in zip(keys, shapes, factors):
        level = out[key]
        assert {d: level.sizes[d] for d in sdims} == shp
        assert si.get_spacing_from_sim(level) == pytest.approx({d: osp0["spacing"][d] * f[d] for d in sdims})
        assert si.get_origin_from_sim(level) == pytest.approx({d: osp0["origin"][d] + (f[d] - 1) * osp0["spacing"][d] / 2 for d in sdims})
    # every level is fused from the input level of its own spacing, not downsampled from the level above
    assert [si.get_spacing_from_sim(c["sims"][0])["x"] for c in stand_in.calls] == [1.0, 2.0]


# ---- errors ----------------------------------------------------------------------------------------------------------------

def _marked_store(tmp_path):
    url = tmp_path / "out.zarr"
    url.mkdir()
    (url / "marker").write_text("an existing store")
    return str(url)


def test_argument_errors(stand_in):
    views, sdims = _mosaic(2)
    with pytest.raises(TypeError, match=r"fuse\(\) missing 1 required positional argument: 'images'"):
        fusion.fuse(transform_key=KEY)
    with pytest.raises(TypeError, match=r"fuse\(\) got both 'images' and deprecated 'sims'. Use only 'images'."):
        fusion.fuse(views, sims=views, transform_key=KEY)
    with pytest.raises(ValueError, match="images must contain at least one image."):
        fusion.fuse([], transform_key=KEY)
    with pytest.raises(ValueError, match="output_zarr_url streams chunks to disk; it cannot be combined with output_on_backend"):
        fusion.fuse(views, transform_key=KEY, output_zarr_url="unused.zarr", output_on_backend=True)
    with pytest.raises(ValueError, match=r"multiview_stitcher_amd.fusion.fuse only implements backend='hip'"):
        fusion.fuse(views, transform_key=KEY, backend="numpy")
    msim = msi_utils.get_msim_from_sim(views[0])
    with pytest.raises(ValueError, match="All input images must be of the same kind: either all SpatialImages or all MultiscaleSpatialImages."):
        fusion.fuse([msim] + views[1:], transform_key=KEY)
    with pytest.raises(ValueError, match="batch_options drive the block-wise Zarr output of fuse\\(\\); pass output_zarr_url as well"):
        fusion.fuse(views, transform_key=KEY, batch_options={"n_batch": 2})
    si.set_sim_affine(views[0], np.zeros((3, 3)), KEY)
    with pytest.raises(ValueError, match="a view's affine is singular"):
        fusion.fuse(views, transform_key=KEY, output_stack_properties=_stack(_mosaic(2)[0], sdims))
    assert not stand_in.calls
    assert fusion.fuse(sims=_mosaic(2)[0], transform_key=KEY).shape and len(stand_in.calls) == 1      # (the alias alone works)


@pytest.mark.parametrize("kwargs, exc, message", [
    (dict(overlap_in_pixels=2, trim_overlap=False), NotImplementedError,
     "trim_overlap=False assembles untrimmed chunks in memory; it cannot stream to a Zarr store"),
    (dict(zarr_options={"zarr_array_creation_kwargs": {"chunks": [8]}}), ValueError,
     r"zarr_array_creation_kwargs\['chunks'\] \[8\] does not match dims \['y', 'x'\]"),
    (dict(zarr_options={"zarr_array_creation_kwargs": {"chunks": [5, 5]}}), ValueError,
     r"store chunks \[5, 5\] do not tile the fuse chunks \[16, 16\]"),
    (dict(zarr_options={"ome_zarr": True, "ngff_version": "0.5", "zarr_array_creation_kwargs": {"zarr_format": 2}}), ValueError,
     r"zarr_format 2 conflicts with NGFF 0.5 \(which stores Zarr v3 arrays\)"),
    (dict(batch_options={"nbatch": 2}), TypeError, r"unknown batch_options keys \['nbatch'\]"),
    (dict(batch_options={"n_batch": 2}, chunk_filter=lambda bi: True), ValueError,
     "batch_options and chunk_filter both select blocks; use one of them"),
], ids=["untrimmed", "chunks-rank", "chunks-tile", "zarr-format", "batch-keys", "batch-filter"])
def test_argument_errors_leave_an_existing_store_untouched(stand_in, tmp_path, kwargs, exc, message):
    views, sdims = _mosaic(2)
    url = _marked_store(tmp_path)
    with pytest.raises(exc, match=message):
        fusion.fuse(views, transform_key=KEY, output_chunksize={"y": 16, "x": 16}, output_zarr_url=url, **kwargs)
    assert os.listdir(url) == ["marker"] and not stand_in.calls
