"""registration.register's host driver without a GPU, through its public seam: a recording ``pairwise_executor(msims, edges,
register_kwargs)`` answers every edge, so what is checked is what the driver DECIDES -- which pairs, which fields of which channel and
time point, which keywords, which edges survive the quality filter, which resolution route, what is written back.  The mosaics are
the test's own: tile ``v`` needs the correction ``OFFSETS[v]`` (times ``1 + it`` at time point ``it``), the executor answers edge
``(i, j)`` with the translation ``offset_i - offset_j`` (the convention of ``resolve_translations``: ``tau_j - tau_i = -d_ij``), so
the resolved parameters are the offsets relative to view 0 whatever route resolves them.  Only the host entry points of the library
(graph pruning, translation resolution) run; ``register_pair_of_msims`` is driven with stand-in registration functions."""
import numpy as np
import pytest

from multiview_stitcher_amd import _lib, _reg_ops, msi_utils, mv_graph, param_resolution, registration
from multiview_stitcher_amd import spatial_image_utils as si

KEY = "stage"
ALL_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
OFFSETS = np.array([[0.5, 0.0, 0.0], [-0.25, 0.5, -1.25], [1.0, -2.0, 0.75], [0.0, 1.5, 2.0]])      # (z, y, x) per view
BASE = np.array([[0.0, 0.0, 0.0], [0.5, -1.0, 0.25], [0.0, 1.0, 0.25], [-0.5, 0.5, -0.5]])         # the views' translations under KEY
ABS_TOL = 1e-6
SOLVER = {"reference_view": 0, "abs_tol": ABS_TOL, "rel_tol": 1e-12, "max_iter": 2000}


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    """Any attempt to initialise a device fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "init", refuse)


def _mosaic(ndim, n_c=0, n_t=0, t_stacked=(), tile=(6, 20, 24), scale_factors=None):
    """2 x 2 (x 1 in z) tiles that overlap by a fifth.  Voxels of view ``v``, channel ``c``, time point ``t`` hold
    ``1000 * c + 100 * t + v + 1``.  View ``v`` is translated by ``BASE[v]`` under KEY; for the views in ``t_stacked`` that affine
    is stacked over the time points (its x translation grows by 0.25 per time point).  ``scale_factors``: multiscale images."""
    sdims = ["z", "y", "x"][-ndim:]
    tile, spacing = tile[-ndim:], (2.0, 1.0, 0.5)[-ndim:]
    views = []
    for v, idx in enumerate(np.ndindex(*((1,) * (ndim - 2) + (2, 2)))):
        ns = ([n_c] if n_c else []) + ([n_t] if n_t else [])
        data = np.empty(tuple(ns) + tuple(tile), np.uint16)
        for c in range(n_c or 1):
            for t in range(n_t or 1):
                data[((c,) if n_c else ()) + ((t,) if n_t else ())] = 1000 * c + 100 * t + v + 1
        origin = {d: i * int(n * 0.8) * sp for d, i, n, sp in zip(sdims, idx, tile, spacing)}
        sim = si.to_spatial_image(data, dims=(["c"] if n_c else []) + (["t"] if n_t else []) + sdims, scale=dict(zip(sdims, spacing)),
                                  translation=origin, c_coords=["dapi", "gfp", "rfp"][:n_c] if n_c else None)
        affine = np.eye(ndim + 1)
        affine[:ndim, ndim] = BASE[v][-ndim:]
        if v in t_stacked:
            affine = np.stack([affine] * n_t)
            affine[:, ndim - 1, ndim] += 0.25 * np.arange(n_t)
        si.set_sim_affine(sim, affine, KEY)
        views.append(msi_utils.get_msim_from_sim(sim, scale_factors=scale_factors) if scale_factors is not None else sim)
    return views


def _offset(v, ndim, it=0):
    return OFFSETS[v][-ndim:] * (1 + it)


def _translation(vec):
    m = np.eye(len(vec) + 1)
    m[:-1, -1] = vec
    return m


def _world_box(field):
    """(lower, upper) of a field under KEY at time point 0: the test's own arithmetic on the coordinates."""
    sim = msi_utils.get_sim_from_msim(field) if msi_utils.is_msim(field) else field
    sdims = [d for d in sim.dims if d in "zyx"]
    t = np.asarray(sim.attrs["transforms"][KEY])
    t = (t[0] if t.ndim == 3 else t)[:-1, -1]
    return (np.array([sim.coords[d][0] for d in sdims]) + t, np.array([sim.coords[d][-1] for d in sdims]) + t)


class Recorder:
    """pairwise_executor: records its arguments; edge (i, j) of call ``it`` is answered with the translation
    ``offset_i - offset_j`` at that time point, ``qualities.get((i, j), 0.9)`` and the intersection of the two world boxes."""

    def __init__(self, qualities=None, reads_only=None, n_results=None):
        self.calls, self.qualities, self.n_results = [], qualities or {}, n_results
        if reads_only is not None:
            self.reads_only = reads_only

    def __call__(self, msims, edges, register_kwargs):
        it = len(self.calls)
        self.calls.append({"msims": msims, "edges": edges, "kwargs": register_kwargs})
        out = []
        for i, j in edges:
            (lo_i, up_i), (lo_j, up_j) = _world_box(msims[i]), _world_box(msims[j])
            ndim = len(lo_i)
            out.append({"transform": _translation(_offset(i, ndim, it) - _offset(j, ndim, it)), "quality": self.qualities.get((i, j), 0.9),
                        "bbox": np.array([np.maximum(lo_i, lo_j), np.minimum(up_i, up_j)])})
        return out if self.n_results is None else out[:self.n_results]


def _register(views, executor=None, **kw):
    executor = executor if executor is not None else Recorder()
    kw.setdefault("groupwise_resolution_kwargs", dict(SOLVER))
    return registration.register(views, transform_key=KEY, pairwise_executor=executor, **kw), executor


def _assert_offsets(params, ndim, it=None):
    """The parameters are the offsets relative to view 0, within the bound the solver was told to stop at."""
    for v, p in enumerate(params):
        for k in range(len(p) if it is None and np.ndim(p) == 3 else 1):
            m = p[k] if np.ndim(p) == 3 else p
            want = _translation(_offset(v, ndim, k if it is None else it) - _offset(0, ndim, k if it is None else it))
            assert m.shape == want.shape and np.abs(m - want).max() <= ABS_TOL, (v, k, m, want)


# ---- edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [2, 3])
def test_the_executor_gets_sorted_pairs_and_both_graph_routes_give_the_same_list(monkeypatch, ndim):
    lists, generic = {}, []
    build = mv_graph.build_view_adjacency_graph
    monkeypatch.setattr(mv_graph, "build_view_adjacency_graph", lambda *a, **k: generic.append(1) or build(*a, **k))
    for native in (True, False):
        monkeypatch.setattr(registration, "_native_graph", [native])
        for name, kw in (("default", {}), ("pairs", {"pairs": [(2, 3), (1, 0)]}), ("unpruned", {"pre_registration_pruning_method": None})):
            del generic[:]
            _, rec = _register(_mosaic(ndim), **kw)
            assert len(rec.calls) == 1 and (name != "default" or len(generic) == (0 if native else 1))     # both routes are taken
            edges = rec.calls[0]["edges"]
            assert all(isinstance(e, tuple) and len(e) == 2 and e[0] < e[1] for e in edges) and len(set(edges)) == len(edges)
            lists[native, name] = [tuple(int(v) for v in e) for e in edges]
    for name in ("default", "pairs", "unpruned"):
        assert lists[True, name] == lists[False, name]
    assert sorted(lists[True, "unpruned"]) == ALL_PAIRS                 # every two tiles of the 2 x 2 mosaic share a corner
    assert sorted(lists[True, "pairs"]) == [(0, 1), (2, 3)]
    assert set(lists[True, "default"]) < set(ALL_PAIRS)                 # the default pruning drops pairs


# ---- executor keywords ----------------------------------------------------------------------------------------------------------
DEFAULT_KEYS = {"transform_key", "registration_binning", "overlap_tolerance", "pairwise_reg_func", "pairwise_reg_func_kwargs"}


@pytest.mark.parametrize("extra", [{}, {"reg_res_level": 0}, {"overlap_bbox": "reference"}, {"points_key": "few"}, {"prefilter_markers": True}],
                         ids=["default", "reg_res_level", "overlap_bbox", "points_key", "prefilter_markers"])
def test_the_executor_gets_the_default_keywords_and_each_option_adds_its_own(extra):
    func_kwargs = {"upsample_factor": 4}
    _, rec = _register(_mosaic(2), registration_binning={"y": 2, "x": 1}, overlap_tolerance=0.5, pairwise_reg_func_kwargs=func_kwargs, **extra)
    kw = rec.calls[0]["kwargs"]
    assert set(kw) == DEFAULT_KEYS | set(extra)
    assert kw["transform_key"] == KEY and kw["registration_binning"] == {"y": 2, "x": 1} and kw["overlap_tolerance"] == 0.5
    assert kw["pairwise_reg_func"] is registration.phase_correlation_registration and kw["pairwise_reg_func_kwargs"] is func_kwargs
    for k, v in extra.items():
        assert kw[k] == v


def test_an_executor_that_returns_too_few_results_is_refused():
    with pytest.raises(ValueError) as e:
        _register(_mosaic(2), Recorder(n_results=2))
    assert str(e.value) == "pairwise_executor must return one result per edge"


# ---- channel --------------------------------------------------------------------------------------------------------------------
def test_two_channels_need_a_choice_and_the_name_wins_over_the_index():
    with pytest.raises(Exception) as e:
        _register(_mosaic(3, n_c=2))
    assert type(e.value) is Exception and str(e.value) == "Please choose a registration channel."
    for kw, c in (({"reg_channel_index": 1}, 1), ({"reg_channel_index": 0}, 0), ({"reg_channel": "gfp"}, 1),
                  ({"reg_channel": "dapi", "reg_channel_index": 1}, 0)):
        views = _mosaic(3, n_c=2)
        _, rec = _register(views, **kw)
        for v, f in enumerate(rec.calls[0]["msims"]):
            assert f.dims == ("z", "y", "x") and np.all(f.data == 1000 * c + v + 1)
        assert all(s.dims == ("c", "z", "y", "x") for s in views)


def test_one_channel_needs_no_choice():
    _, rec = _register(_mosaic(2, n_c=1))
    for v, f in enumerate(rec.calls[0]["msims"]):
        assert f.dims == ("y", "x") and np.all(f.data == v + 1)


# ---- time -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [2, 3])
def test_every_time_point_gets_its_own_fields_and_the_callers_images_stay_as_they_are(ndim):
    views = _mosaic(ndim, n_t=3, t_stacked=(1,))
    before = [(s, s.data, s.attrs["transforms"], s.attrs["transforms"][KEY]) for s in views]
    params, rec = _register(views, new_transform_key=None)
    assert len(rec.calls) == 3
    for it, call in enumerate(rec.calls):
        for v, f in enumerate(call["msims"]):
            assert "t" not in f.dims and np.all(f.data == 100 * it + v + 1)
            got = f.attrs["transforms"][KEY]
            assert got.shape == (ndim + 1, ndim + 1) and np.array_equal(got, before[v][3][it] if v == 1 else before[v][3])
    assert all(p.shape == (3, ndim + 1, ndim + 1) for p in params)
    _assert_offsets(params, ndim)
    for s, (s0, data, transforms, affine) in zip(views, before):
        assert s is s0 and s.data is data and s.attrs["transforms"] is transforms and s.attrs["transforms"][KEY] is affine
        assert s.dims[0] == "t" and s.sizes["t"] == 3 and list(transforms) == [KEY]
    assert views[1].attrs["transforms"][KEY].shape == (3, ndim + 1, ndim + 1)


# ---- copies ---------------------------------------------------------------------------------------------------------------------
def test_a_reading_executor_gets_the_images_themselves_any_other_gets_copies():
    views = _mosaic(3)
    _, rec = _register(views, Recorder(reads_only=True), new_transform_key=None)
    assert all(f is s for f, s in zip(rec.calls[0]["msims"], views))
    for executor in (Recorder(), Recorder(reads_only=False)):
        _, rec = _register(views, executor, new_transform_key=None)
        for f, s in zip(rec.calls[0]["msims"], views):
            assert f is not s and f.attrs["transforms"] is not s.attrs["transforms"] and f.data is s.data
            assert np.array_equal(f.attrs["transforms"][KEY], s.attrs["transforms"][KEY])
    # a t-stacked affine on an image without t is something to select: copies even for a reading executor
    stacked = np.stack([views[2].attrs["transforms"][KEY]] * 2)
    si.set_sim_affine(views[2], stacked, KEY)
    _, rec = _register(views, Recorder(reads_only=True), new_transform_key=None)
    fields = rec.calls[0]["msims"]
    assert fields[2] is not views[2] and fields[2].attrs["transforms"][KEY].shape == (4, 4) and fields[0] is views[0]
    assert views[2].attrs["transforms"][KEY] is not None and views[2].attrs["transforms"][KEY].shape == (2, 4, 4)


# ---- quality filter -------------------------------------------------------------------------------------------------------------
class Resolver:
    """A callable groupwise_resolution_method: records the edges of the graph it is handed, resolves nothing."""

    def __init__(self):
        self.edges = []

    def __call__(self, g, **kwargs):
        self.edges += list(g.edges)
        return {n: np.eye(g.ndim + 1) for n in g.nodes}, None


@pytest.mark.parametrize("do_filter,want", [(True, [e for e in ALL_PAIRS if e != (0, 1)]), (False, ALL_PAIRS)])
def test_the_quality_filter_drops_what_is_below_the_threshold_and_keeps_nan(do_filter, want):
    resolver = Resolver()
    qualities = {(0, 1): 0.1, (2, 3): np.nan, (0, 2): 0.2}
    out, rec = _register(_mosaic(2), Recorder(qualities), pre_registration_pruning_method=None, groupwise_resolution_method=resolver,
                         groupwise_resolution_kwargs={}, post_registration_do_quality_filter=do_filter,
                         post_registration_quality_threshold=0.2, return_dict=True)
    assert sorted(resolver.edges) == want
    # the filter touches what is resolved, not what is reported
    assert sorted(out["pairwise_registration"]["edges"]) == ALL_PAIRS and len(out["pairwise_registration"]["results"][0]) == 6


# ---- resolution routes ----------------------------------------------------------------------------------------------------------
class Routes:
    """Recording wrappers around the three resolvers; ``groupwise_resolution`` is handed on without the keyword ``extra``."""

    def __init__(self, monkeypatch):
        self.taken = []
        for module, name in ((registration, "resolve_translations"), (param_resolution, "resolve_translations_native"),
                             (param_resolution, "groupwise_resolution")):
            monkeypatch.setattr(module, name, self._wrap(name, getattr(module, name)))

    def _wrap(self, name, inner):
        def wrapped(*a, **k):
            self.taken.append((name, dict(k)))
            k.pop("extra", None)
            return inner(*a, **k)
        return wrapped


ROUTE_CASES = {      # method, _native_resolution, extra kwargs -> the resolver reached
    "linear": ("linear", True, {}, "resolve_translations"),
    "native": ("global_optimization", True, {}, "resolve_translations_native"),
    "native_off": ("global_optimization", False, {}, "groupwise_resolution"),
    "extra_kwarg": ("global_optimization", True, {"extra": 1}, "groupwise_resolution"),
}


@pytest.mark.parametrize("ndim,n_t", [(2, 0), (3, 2)], ids=["2d", "3d_t2"])
@pytest.mark.parametrize("case", list(ROUTE_CASES))
def test_every_resolution_route_is_reached_and_returns_the_true_offsets(monkeypatch, case, ndim, n_t):
    method, native, extra, want = ROUTE_CASES[case]
    monkeypatch.setattr(registration, "_native_resolution", [native])
    routes = Routes(monkeypatch)
    out, rec = _register(_mosaic(ndim, n_t=n_t), groupwise_resolution_method=method, groupwise_resolution_kwargs=dict(SOLVER, **extra),
                         return_dict=True)
    nt = max(n_t, 1)
    assert [name for name, _ in routes.taken] == [want] * nt
    if want != "resolve_translations":
        assert all(k == dict(SOLVER, **extra) for _, k in routes.taken)
    _assert_offsets(out["params"], ndim)
    info, results = out["groupwise_resolution"]["info"], out["pairwise_registration"]["results"]
    assert len(info) == nt and all((i is None) == (method == "linear") for i in info)
    assert len(results) == nt == len(rec.calls)
    for it, res in enumerate(results):      # each time point's results once, in the executor's order
        assert len(res) == len(rec.calls[it]["edges"])
        for (i, j), r in zip(rec.calls[it]["edges"], res):
            assert np.array_equal(r["transform"], _translation(_offset(i, ndim, it) - _offset(j, ndim, it)))


# ---- write-back -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale_factors", [None, [], [2]], ids=["sims", "msims_scale0", "msims_two_levels"])
def test_the_new_key_holds_the_parameters_rebased_on_the_old_one(scale_factors):
    views = _mosaic(3, scale_factors=scale_factors)
    params, rec = _register(views, new_transform_key="registered")
    _assert_offsets(params, 3)
    if scale_factors:
        assert all(msi_utils.is_msim(f) and f.keys() == ["scale0", "scale1"] for f in rec.calls[0]["msims"])
    for v, (m, p) in enumerate(zip(views, params)):
        holders = [m.attrs["transforms"]] if scale_factors is None else [m.transforms] + [s.attrs["transforms"] for s in m.scales.values()]
        for transforms in holders:
            assert set(transforms) == {KEY, "registered"}
            want = _translation(BASE[v] + p[:3, 3])             # two pure translations: their sum
            assert np.abs(transforms["registered"] - want).max() <= 1e-12
            assert np.array_equal(transforms[KEY], _translation(BASE[v]))


def test_without_a_new_key_nothing_is_written():
    for scale_factors in (None, [2]):
        views = _mosaic(2, scale_factors=scale_factors)
        _register(views, new_transform_key=None)
        for m in views:
            assert list(m.attrs["transforms"] if scale_factors is None else m.transforms) == [KEY]


# ---- return_dict ----------------------------------------------------------------------------------------------------------------
def test_the_report_has_its_keys_and_the_qualities_by_edge():
    qualities = {(0, 1): 0.3, (2, 3): 0.7}
    out, rec = _register(_mosaic(2), Recorder(qualities), return_dict=True)
    params, _ = _register(_mosaic(2), Recorder(qualities))
    assert set(out) == {"params", "bin_cache_stats", "groupwise_resolution", "pairwise_registration"}
    assert out["bin_cache_stats"] is None                                 # an executor: no binned tiles of the call's own
    assert set(out["groupwise_resolution"]) == {"info"} and set(out["pairwise_registration"]) == {"edges", "results", "metrics"}
    edges = out["pairwise_registration"]["edges"]
    assert edges == rec.calls[0]["edges"]
    assert out["pairwise_registration"]["metrics"] == {"qualities": {e: qualities.get(e, 0.9) for e in edges}}
    assert isinstance(params, list) and all(np.array_equal(a, b) for a, b in zip(params, out["params"]))


# ---- upload gate ----------------------------------------------------------------------------------------------------------------
def _gate_call(views, **kw):
    """The call frame as register() has it when it asks the gate."""
    arguments = dict(msims=views, reg_channel=None, reg_channel_index=None, pairwise_executor=None, reg_res_level=None,
                     pairwise_reg_func=registration.phase_correlation_registration, pairwise_reg_func_kwargs=None, device=0)
    call = registration._RegisterCall(**dict(arguments, **kw))
    registration._registration_channel(call)
    registration._pyramid_levels(call)
    return call


def _big_views(rows):
    """Four 2-D uint16 tiles of ``rows[v]`` x 8192 that own one sample each (broadcast views: 16 KiB a row as the gate counts them)."""
    views = []
    for v, n in enumerate(rows):
        sim = si.to_spatial_image(np.broadcast_to(np.zeros((1, 1), np.uint16), (n, 8192)), dims=["y", "x"], scale={"y": 1.0, "x": 1.0},
                                  translation={"y": 0.0, "x": 6000.0 * v})
        si.set_sim_affine(sim, np.eye(3), KEY)
        views.append(sim)
    return views


def test_the_upload_gate_opens_at_256_mib_of_plain_host_tiles_for_the_built_in_pair_path(monkeypatch):
    asked = []
    monkeypatch.setattr(_lib, "device_count", lambda: asked.append(1) or 1)
    monkeypatch.setattr(registration, "_HOST_UPLOAD_ASYNC", [True])
    at, below = [4096] * 4, [4096, 4096, 4096, 4095]                # 4 x 4096 x 8192 x 2 bytes = 256 MiB
    assert registration._wants_async_upload(_gate_call(_big_views(at))) is True and len(asked) == 1
    # ... and with keywords for the built-in function: the gate does not look at them
    assert registration._wants_async_upload(_gate_call(_big_views(at), pairwise_reg_func_kwargs={"disambiguate_region_mode": "corr"}))
    del asked[:]
    closed = [
        _gate_call(_big_views(below)),
        _gate_call([msi_utils.get_msim_from_sims([v, v.isel({"y": slice(0, None, 2), "x": slice(0, None, 2)})]) for v in _big_views(at)]),
        _gate_call(_big_views(at), pairwise_reg_func=lambda fixed_data, moving_data: None),
        _gate_call(_big_views(at), pairwise_executor=Recorder()),
        _gate_call(_big_views(at), reg_res_level=0),
    ]
    for call in closed:
        assert not registration._wants_async_upload(call)
    assert not asked                                                 # the device count is asked after all of these
    monkeypatch.setattr(registration, "_HOST_UPLOAD_ASYNC", [False])
    assert not registration._wants_async_upload(_gate_call(_big_views(at))) and not asked


# ---- register_pair_of_msims -----------------------------------------------------------------------------------------------------
def _pair(far=False):
    a, b = _mosaic(3)[:2]
    if far:
        si.set_sim_affine(b, _translation([0.0, 0.0, 1e4]), KEY)
    for s in (a, b):
        si.set_point_set(s, np.zeros((1, 3)))
    return a, b


def _by_points(fixed_points, moving_points):
    return {"affine_matrix": _translation([0.0, 1.0, 2.0]), "quality": 0.5}


def _by_pixels(fixed_data, moving_data):
    return {"affine_matrix": _translation([0.0, 1.0, 2.0]), "quality": None}


@pytest.fixture
def host_pixels(monkeypatch):
    """The two device steps of the pixel body as host stand-ins: the crops as they are (their grids need not coincide: the stand-in
    registration functions do not look at the voxels), and numpy's minimum and maximum for the constant-image guard."""
    seen = []

    def crops_as_they_are(sim1, sim2, transform_key, overlap_bboxes, device=0):
        seen.append((sim1, sim2, overlap_bboxes))
        return sim1, sim2

    monkeypatch.setattr(registration, "sims_to_intrinsic_coord_system", crops_as_they_are)
    monkeypatch.setattr(_reg_ops, "rescale_intensity", lambda im, device, out_on_device=False: (None, float(np.min(im)), float(np.max(im)), None))
    return seen


def test_an_unknown_overlap_bbox_is_refused():
    a, b = _pair()
    for func in (_by_points, _by_pixels):
        with pytest.raises(ValueError) as e:
            registration.register_pair_of_msims(a, b, KEY, pairwise_reg_func=func, overlap_bbox="qhull")
        assert str(e.value) == "overlap_bbox must be 'closed_form' or 'reference'"


@pytest.mark.parametrize("overlap_bbox", ["closed_form", "reference"])
def test_views_that_do_not_overlap_are_refused(overlap_bbox):
    a, b = _pair(far=True)
    for func in (_by_points, _by_pixels):
        with pytest.raises(ValueError) as e:
            registration.register_pair_of_msims(a, b, KEY, pairwise_reg_func=func, overlap_bbox=overlap_bbox)
        assert str(e.value) == "views do not overlap"


@pytest.mark.parametrize("overlap_bbox", ["closed_form", "reference"])
def test_the_pixel_body_and_the_point_body_report_the_same_box(host_pixels, overlap_bbox):
    a, b = _pair()
    points = registration.register_pair_of_msims(a, b, KEY, pairwise_reg_func=_by_points, overlap_bbox=overlap_bbox)
    assert not host_pixels
    a.data[:] = np.arange(a.data.shape[-1])                           # (not constant: the guard lets the function run)
    b.data[:] = np.arange(b.data.shape[-1])
    pixels = registration.register_pair_of_msims(a, b, KEY, pairwise_reg_func=_by_pixels, overlap_bbox=overlap_bbox)
    assert len(host_pixels) == 1
    assert set(points) == set(pixels) == {"transform", "quality", "bbox"}
    assert pixels["bbox"].shape == (2, 3) and np.array_equal(points["bbox"], pixels["bbox"])
    # the box is the intersection of the two world boxes (within the round-off of the reference's vertices)
    (lo_a, up_a), (lo_b, up_b) = _world_box(a), _world_box(b)
    assert np.abs(pixels["bbox"] - [np.maximum(lo_a, lo_b), np.minimum(up_a, up_b)]).max() <= 1e-9
    assert points["quality"] == 0.5 and np.isnan(pixels["quality"])   # no quality: NaN
    assert np.array_equal(points["transform"], _translation([0.0, 1.0, 2.0]))      # the point body's transform is physical as it is


def test_a_list_from_the_registration_function_is_an_error(host_pixels):
    a, b = _pair()
    a.data[:] = np.arange(a.data.shape[-1])
    b.data[:] = np.arange(b.data.shape[-1])
    with pytest.raises(RuntimeError) as e:
        registration.register_pair_of_msims(a, b, KEY, pairwise_reg_func=lambda fixed_data, moving_data: [np.zeros(3)])
    assert str(e.value) == "phase correlation produced no admissible shift candidate (registration.py:479-480)"
