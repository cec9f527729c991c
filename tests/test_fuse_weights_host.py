"""CPU: the host side of ``view_weights``: the properties of its oracle (tests/mask_fuse_oracle.py) against ``oracle.fuse_oracle``,
what fusion.fuse's driver hands to ``fuse_np`` under a recording stand-in, and the refusals that need no device."""
import numpy as np
import pytest

from multiview_stitcher_amd import fusion, msi_utils
from multiview_stitcher_amd import spatial_image_utils as si
from multiview_stitcher_amd import weights
from oracle import fuse_oracle as fo
from tests import affine_cases as ac
from tests import fuse_weight_cases as wc
from tests import mask_fuse_oracle as mfo
from tests.helpers import same_bits, sim_to_view

KEY = "k"
FUSIONS = ("weighted_average", "max", "simple_average")


def _case(name, dtype=np.uint16):
    sims, params, out_bb, kw = ac.build(name, dtype)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    return list(views), list(params), out_bb, list(bbs), kw


def _tiles(views, datas):
    return [None if d is None else dict(v, data=d) for v, d in zip(views, datas)]


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fusion_name", FUSIONS)
@pytest.mark.parametrize("name", ["fan2d_12", "trimmed"])
def test_full_weights_reproduce_the_plain_oracle(name, fusion_name):
    views, params, out_bb, bbs, kw = _case(name)
    want, want_f, _ = ac.oracle(name, np.uint16, fusion_name, 1)
    full = _tiles(views, [np.full(v["data"].shape, 252, np.uint8) for v in views])
    got, got_f, dbg = mfo.fuse_np(views, params, out_bb, full, fusion=fusion_name, full_view_bbs=bbs, **kw)
    assert same_bits(got, want) and same_bits(got_f, want_f) and np.all(dbg["m"] == 1)
    none = mfo.fuse_np(views, params, out_bb, [None] * len(views), fusion=fusion_name, full_view_bbs=bbs, **kw)
    assert same_bits(none[1], want_f)
    over = _tiles(views, [np.full(v["data"].shape, 255, np.uint8) for v in views])          # above 252 counts as 252
    assert same_bits(mfo.fuse_np(views, params, out_bb, over, fusion=fusion_name, full_view_bbs=bbs, **kw)[1], want_f)


@pytest.mark.parametrize("fusion_name", FUSIONS)
def test_a_view_with_an_all_zero_tile_disappears(fusion_name):
    views, params, out_bb, bbs, kw = _case("shear_aniso")
    datas = [None, np.zeros(views[1]["data"].shape, np.uint8), None]
    got = mfo.fuse_np(views, params, out_bb, _tiles(views, datas), fusion=fusion_name, full_view_bbs=bbs, **kw)[1]
    keep = [0, 2]
    want = fo.fuse_np([views[i] for i in keep], [params[i] for i in keep], out_bb, fusion=fusion_name, full_view_bbs=[bbs[i] for i in keep],
                      return_float=True, **kw)[1]
    assert same_bits(got, want)
    assert not same_bits(want, ac.oracle("shear_aniso", np.uint16, fusion_name, 1)[1])      # (the view did contribute)


@pytest.mark.parametrize("fusion_name", FUSIONS)
def test_a_fully_masked_voxel_is_zero_and_the_feather_shows(fusion_name):
    views, params, out_bb, bbs, kw = _case("fan2d_12")
    tiles = _tiles(views, wc.feathered_tiles("fan2d_12"))
    got, got_f, dbg = mfo.fuse_np(views, params, out_bb, tiles, fusion=fusion_name, full_view_bbs=bbs, **kw)
    plain_views = ac.oracle("fan2d_12", np.uint16, fusion_name, 1)[2]["views"]
    covered, masked = ~np.isnan(plain_views), np.isnan(dbg["views"])
    lost = covered.any(0) & masked.all(0)                      # covered by a view, but every covering view is masked out there
    assert lost.sum() > 20 and np.all(got_f[lost] == 0) and np.all(got[lost] == 0)
    assert np.all(got_f[~masked.all(0)] > 0)                   # (white noise of uint16: a voxel some view reaches is positive)
    assert wc.feather_shows(dbg["m"], dbg["views"]) > 0.05 and (got != 0).mean() > 0.3
    if fusion_name == "weighted_average":
        # where exactly two views take part, the result lies between them and moves towards the view whose tile weight is larger
        two = (~masked).sum(0) == 2
        pair = dbg["views"][:, two]
        assert np.all(got_f[two] >= np.nanmin(pair, 0) - 1e-2) and np.all(got_f[two] <= np.nanmax(pair, 0) + 1e-2)


# ---- fuse()'s driver under a recording stand-in ----------------------------------------------------------------------------------------
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
    monkeypatch.setattr(fusion, "_resident_weight", lambda data, device: data)      # (no device: the "uploaded" tile is the tile)
    return rec


def _mosaic(ndim):
    """2 x 2 (x 1 in z) tiles; the voxels of view ``iv`` hold ``iv + 1``, the weight tile of view ``iv`` holds ``10 + iv``."""
    sdims = ["z", "y", "x"][-ndim:]
    tile = (12, 40, 48)[-ndim:]
    views, tiles = [], []
    for iv, idx in enumerate(np.ndindex(*((1,) * (ndim - 2) + (2, 2)))):
        origin = {d: float(i * int(n * 0.8)) for d, i, n in zip(sdims, idx, tile)}
        sim = si.to_spatial_image(np.full(tile, iv + 1, np.uint16), dims=sdims, scale={d: 1.0 for d in sdims}, translation=origin)
        si.set_sim_affine(sim, np.eye(ndim + 1), KEY)
        views.append(sim)
        tiles.append(si.to_spatial_image(np.full(tile, 10 + iv, np.uint8), dims=sdims, scale={d: 1.0 for d in sdims}, translation=origin))
    return views, tiles, sdims


@pytest.mark.parametrize("ndim", [2, 3])
def test_every_call_carries_the_tiles_of_exactly_its_views(stand_in, ndim):
    views, tiles, sdims = _mosaic(ndim)
    given = [tiles[0], None, np.asarray(tiles[2].data), tiles[3]]             # a sim, no tile, a plain array, a sim
    chunks = {d: 30 for d in sdims}
    fusion.fuse(views, transform_key=KEY, output_chunksize=chunks, merge_chunks=False, view_weights=given)
    assert len(stand_in.calls) >= 4
    seen = set()
    for kw in stand_in.calls:
        ids = [int(np.asarray(s.data).flat[0]) - 1 for s in kw["sims"]]
        assert ids == sorted(ids) and len(kw["view_weights"]) == len(ids)
        seen.update(ids)
        for iv, w in zip(ids, kw["view_weights"]):
            if iv == 1:
                assert w is None
                continue
            data = w.data if isinstance(w, si.SpatialImage) else w
            assert tuple(data.shape) == tuple(views[iv].data.shape) and int(np.asarray(data).flat[0]) == 10 + iv      # the WHOLE tile of this view
            assert isinstance(w, si.SpatialImage) == (iv != 2)
            if iv != 2:
                for d in sdims:
                    assert np.array_equal(np.asarray(w.coords[d]), np.asarray(tiles[iv].coords[d]))
    assert seen == {0, 1, 2, 3}
    n_split = len(stand_in.calls)
    stand_in.calls.clear()
    fusion.fuse(views, transform_key=KEY, output_chunksize=chunks, view_weights=given)      # merged launch blocks carry them as well
    assert 1 <= len(stand_in.calls) < n_split and all("view_weights" in kw for kw in stand_in.calls)


@pytest.mark.parametrize("merge", [True, False])
def test_no_keyword_when_none_was_given(stand_in, merge):
    views, _, sdims = _mosaic(2)
    fusion.fuse(views, transform_key=KEY, output_chunksize={d: 30 for d in sdims}, merge_chunks=merge)
    assert stand_in.calls and all("view_weights" not in kw for kw in stand_in.calls)
    stand_in.calls.clear()
    fusion.fuse(views, transform_key=KEY, output_chunksize={d: 30 for d in sdims}, merge_chunks=merge, view_weights=None)
    assert stand_in.calls and all("view_weights" not in kw for kw in stand_in.calls)


def test_launch_budget_counts_the_tiles_to_upload(monkeypatch):
    views, tiles, sdims = _mosaic(3)
    free = 1 << 30
    monkeypatch.setattr(fusion._lib, "mem_info", lambda device: (free, free))
    shape = {d: 100 for d in sdims}
    plain = fusion._launch_budget(views, shape, sdims, 2, 0, 1 << 40)
    with_tiles = fusion._launch_budget(views, shape, sdims, 2, 0, 1 << 40, view_weights=[tiles[0], None, np.asarray(tiles[2].data), None])
    n_tile = int(np.prod(views[0].data.shape))
    staged = sum(int(np.prod(v.data.shape)) * 2 for v in views)
    per_out_byte = 1.0 + 2.0 * staged / (100 ** 3 * 2)
    assert plain == int((int(0.9 * free) - n_tile * 2) / per_out_byte)
    assert with_tiles == int((int(0.9 * free) - n_tile * 2 - 2 * n_tile) / per_out_byte)
    assert fusion._weight_upload_bytes(None, 0) == 0


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def _user_fusion(transformed_views=None):
    return np.nanmin(transformed_views, axis=0)


REFUSED = [
    (dict(weights_func=fusion.content_based), "weights_func"),
    (dict(weights_func=weights.content_based_dct), "weights_func"),
    (dict(fusion_func=fusion.multi_view_deconvolution), "multi_view_deconvolution"),
    (dict(fusion_func=fusion.multi_band_fusion), "multi_band_fusion"),
    (dict(fusion_func=_user_fusion), "user callable"),
]


@pytest.mark.parametrize("kwargs,word", REFUSED)
def test_combinations_are_refused_by_name_at_call_time(stand_in, kwargs, word):
    views, tiles, _ = _mosaic(2)
    with pytest.raises(NotImplementedError, match=word):
        fusion.fuse(views, transform_key=KEY, view_weights=tiles, **kwargs)
    assert not stand_in.calls
    with pytest.raises(NotImplementedError, match=word):      # (the check fuse_np itself makes; the function is replaced here)
        fusion._check_view_weights_call(kwargs.get("fusion_func", fusion.weighted_average_fusion), kwargs.get("weights_func"), "fuse_np")


def test_fuse_np_refuses_before_it_touches_a_device():
    views, tiles, sdims = _mosaic(2)
    box = si.get_stack_properties_from_sim(views[0])
    with pytest.raises(NotImplementedError, match="weights_func"):
        fusion.fuse_np(views[:1], [np.eye(3)], box, weights_func=fusion.content_based, view_weights=tiles[:1])
    with pytest.raises(NotImplementedError, match="multi_band_fusion"):
        fusion.fuse_np(views[:1], [np.eye(3)], box, fusion_func=fusion.multi_band_fusion, view_weights=tiles[:1])
    with pytest.raises(ValueError, match="one entry per view"):
        fusion.fuse_np(views[:2], [np.eye(3)] * 2, box, view_weights=tiles[:1])


def test_tiles_are_checked_against_their_views(stand_in):
    views, tiles, sdims = _mosaic(2)
    with pytest.raises(ValueError, match="one entry per view"):
        fusion.fuse(views, transform_key=KEY, view_weights=tiles[:3])
    per_t = si.to_spatial_image(np.ones((2, 40, 48), np.uint8), dims=["t", "y", "x"], scale={"y": 1.0, "x": 1.0}, translation={"y": 0.0, "x": 0.0})
    with pytest.raises(NotImplementedError, match="'t' dim"):
        fusion.fuse(views, transform_key=KEY, view_weights=[per_t, None, None, None])
    with pytest.raises(ValueError, match="shape"):
        fusion.fuse(views, transform_key=KEY, view_weights=[np.ones((20, 24), np.uint8), None, None, None])      # another grid comes as a sim
    with pytest.raises(TypeError, match="uint8"):
        fusion.fuse(views, transform_key=KEY, view_weights=[np.ones((40, 48), np.float32), None, None, None])
    msims = [msi_utils.get_msim_from_sim(v, scale_factors=[]) for v in views]
    with pytest.raises(NotImplementedError, match="multiscale"):
        fusion.fuse(msims, transform_key=KEY, view_weights=tiles)
    assert not stand_in.calls


def test_plane_wise_blocks_are_refused_by_name(stand_in):
    views, tiles, sdims = _mosaic(3)
    with pytest.raises(NotImplementedError, match="plane-wise"):
        fusion.fuse(views, transform_key=KEY, output_chunksize={"z": 1, "y": 64, "x": 64}, view_weights=tiles)
    stand_in.calls.clear()
    fusion.fuse(views, transform_key=KEY, output_chunksize={"z": 1, "y": 64, "x": 64})        # without tiles the same call is fused plane by plane
    assert stand_in.calls


def test_calls_with_tiles_stay_out_of_the_replay():
    call = fusion._FuseCall(output_on_backend=True, output_zarr_url=None, batch_options=None, chunk_filter=None, merge_chunks=True, weights_func=None,
                            fusion_func_kwargs=None, weights_func_kwargs=None, zarr_options=None, backend="hip", view_weights=[None])
    assert fusion._replay_lookup(call) is None and call.replay_key is None and call.record is None
