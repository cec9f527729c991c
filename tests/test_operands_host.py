"""The operand step of the ctypes wrappers (``_operands.py``) without a GPU and without the library: a stand-in records every
``mvs_*`` call, so what is checked is what the wrappers hand over and in which order -- the pointer and mem code of an input, the
one same-side check, the result frame, and that every wrapper that takes a ``DeviceArray`` makes its stream wait for an upload
still in flight (``mvs_event_wait`` with the array's ticket) BEFORE its entry point is called."""
import numpy as np
import pytest

from multiview_stitcher_amd import (_detect_ops, _label_ops, _lib, _marker_ops, _mask_ops, _masked_corr_ops, _operands, _reg_ops, _shading_ops,
                                    transformation)
from multiview_stitcher_amd.device import DeviceArray, _Pending

SHAPE = (4, 6, 8)
OUT_MESSAGE = "out must be a contiguous DeviceArray of the result shape and dtype"


class RecordingLib:
    """Every ``mvs_*`` attribute records ``(name, args)`` and returns 0; ``mvs_malloc`` hands out made-up addresses."""

    def __init__(self):
        self.calls = []
        self.next_address = 0x100000

    def __getattr__(self, name):
        if not name.startswith("mvs_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            if name == "mvs_malloc":
                args[2]._obj.value = self.next_address
                self.next_address += 0x100000
            if name == "mvs_affine_mi_gradient":      # (its wrapper converts a count it reads back: give it zeros)
                for i in range(_lib.MVS_AFFINE_MI_GRAD_LEN):
                    args[-1][i] = 0.0
            return 0

        return entry

    def names(self):
        return [name for name, _ in self.calls]

    def waited_before(self, entry):
        """The tickets of the ``mvs_event_wait`` calls recorded before the first call of ``entry``, with their devices."""
        first = self.names().index(entry)
        return [(args[0], args[1]) for name, args in self.calls[:first] if name == "mvs_event_wait"]


@pytest.fixture
def lib(monkeypatch):
    """The recording stand-in behind ``_lib.init`` / ``_lib.load``.  The allocations made through it forget their made-up
    addresses afterwards, so that nothing is ever released through the real library."""
    fake = RecordingLib()
    buffers = []
    make = _lib.DeviceBuffer.__init__

    def tracked(self, device, nbytes):
        make(self, device, nbytes)
        buffers.append(self)

    monkeypatch.setattr(_lib, "init", lambda device=0: fake)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    monkeypatch.setattr(_lib.DeviceBuffer, "__init__", tracked)
    yield fake
    for b in buffers:
        b.ptr = None


def settled(shape=SHAPE, dtype=np.float32, address=0x1000, device=0):
    return DeviceArray.from_pointer(address, shape, dtype, device)


def pending(ticket, shape=SHAPE, dtype=np.float32, address=0x1000, device=0):
    """A resident array whose upload (ticket ``ticket``) is still in flight."""
    strides = [int(np.prod(shape[i + 1:])) for i in range(len(shape))]
    return DeviceArray(None, address, shape, strides, dtype, device, pending=_Pending(ticket, None))


# ---- dense_operand, operand_pair ---------------------------------------------------------------------------------------------------
def test_dense_operand_checks_a_device_array_and_hands_over_its_pointer(lib):
    a = settled()
    assert _operands.dense_operand(a, (np.float32,), 0, "x") == (0x1000, _lib.MVS_MEM_DEVICE, a)
    assert lib.calls == []                                                       # settled, on its own device: no library call
    with pytest.raises(TypeError, match="x: .*contiguous"):
        _operands.dense_operand(a[:, 1:], (np.float32,), 0, "x")                 # a strided window
    with pytest.raises(TypeError, match="x: .*float32"):
        _operands.dense_operand(settled(dtype=np.uint16), (np.float32,), 0, "x")
    with pytest.raises(ValueError):
        _operands.dense_operand(a[:, 1:], (np.float32,), 0, "x", error=ValueError)
    assert _operands.dense_operand(settled(dtype=np.uint16), _lib.DTYPE_CODES, 0, "x")[1] == _lib.MVS_MEM_DEVICE
    assert lib.calls == []


def test_dense_operand_makes_a_host_array_contiguous_and_casts_it():
    a = np.arange(48, dtype=np.float64).reshape(6, 8)
    ptr, mem, keep = _operands.dense_operand(a, (np.float32,), 0, "x", host_dtype=np.float32)
    assert mem == _lib.MVS_MEM_HOST and keep.dtype == np.float32 and keep.flags.c_contiguous and ptr == keep.ctypes.data
    assert np.array_equal(keep, a)
    ptr, mem, keep = _operands.dense_operand(a[:, 1:], (np.float32,), 0, "x")     # no host_dtype: the dtype stays
    assert keep.dtype == np.float64 and keep.flags.c_contiguous and np.array_equal(keep, a[:, 1:])
    b = np.zeros(SHAPE, np.float32)
    assert _operands.dense_operand(b, (np.float32,), 0, "x", host_dtype=np.float32)[2] is b      # nothing to do: no copy


def test_dense_operand_waits_once_for_a_pending_upload_and_never_for_a_settled_array(lib):
    _operands.dense_operand(pending(77), (np.float32,), 0, "x")
    assert [(n, a[:2]) for n, a in lib.calls] == [("mvs_event_wait", (0, 77))]
    _operands.dense_operand(pending(78), (np.float32,), 3 << 8, "x")             # lane 3 of the same GPU waits on its own stream
    assert [(n, a[:2]) for n, a in lib.calls][1:] == [("mvs_event_wait", (3 << 8, 78))]
    _operands.dense_operand(settled(), (np.float32,), 0, "x")
    assert len(lib.calls) == 2


def test_operand_pair_shares_one_side(lib):
    a, b = settled(), pending(5, address=0x2000)
    pa, pb, mem, keep = _operands.operand_pair(a, b, (np.float32,), 0, "x")
    assert (pa, pb, mem) == (0x1000, 0x2000, _lib.MVS_MEM_DEVICE) and keep == (a, b)
    assert [(n, args[:2]) for n, args in lib.calls] == [("mvs_event_wait", (0, 5))]
    h = np.zeros(SHAPE, np.float32)
    pa, pb, mem, keep = _operands.operand_pair(h, h + 1, (np.float32,), 0, "x", host_dtype=np.float32)
    assert mem == _lib.MVS_MEM_HOST and pa == keep[0].ctypes.data and pb == keep[1].ctypes.data
    for mixed in ((a, h), (h, a)):
        with pytest.raises(TypeError, match=r"both crops must live on the same side \(host or device\)"):
            _operands.operand_pair(*mixed, (np.float32,), 0, "x", names="crops")
    # an optional operand: the one that is there decides the side, none at all counts as host
    assert _operands.operand_pair(None, a, (np.float32,), 0, "x")[:3] == (None, 0x1000, _lib.MVS_MEM_DEVICE)
    assert _operands.operand_pair(None, None, (np.float32,), 0, "x")[:3] == (None, None, _lib.MVS_MEM_HOST)


# ---- result_array, written -----------------------------------------------------------------------------------------------------------
def test_result_array_allocates_on_the_asked_side(lib):
    out, ptr, mem = _operands.result_array([3, 5], np.uint16, False, 0)
    assert isinstance(out, np.ndarray) and out.shape == (3, 5) and out.dtype == np.uint16 and (ptr, mem) == (out.ctypes.data, _lib.MVS_MEM_HOST)
    assert lib.calls == []
    out, ptr, mem = _operands.result_array((3, 5), np.uint16, True, 0)
    assert isinstance(out, DeviceArray) and out.shape == (3, 5) and out.dtype == np.uint16 and out.is_contiguous()
    assert (ptr, mem) == (out.ptr, _lib.MVS_MEM_DEVICE) and ptr != 0 and lib.names() == ["mvs_malloc"]


def test_result_array_checks_out_once(lib):
    mine = settled((3, 5), np.uint16)
    assert _operands.result_array((3, 5), np.uint16, True, 0, mine) == (mine, mine.ptr, _lib.MVS_MEM_DEVICE)
    host = np.zeros((3, 5), np.uint16)
    assert _operands.result_array((3, 5), np.uint16, False, 0, host) == (host, host.ctypes.data, _lib.MVS_MEM_HOST)
    assert lib.calls == []
    _operands.result_array((3, 5), np.uint16, True, 0, pending(9, (3, 5), np.uint16))      # an upload into out still in flight
    assert [(n, a[:2]) for n, a in lib.calls] == [("mvs_event_wait", (0, 9))]
    bad = {"shape": settled((3, 6), np.uint16), "dtype": settled((3, 5), np.float32), "strided": settled((3, 6), np.uint16)[:, 1:], "kind": host}
    assert bad["strided"].shape == (3, 5) and not bad["strided"].is_contiguous()
    for out in bad.values():
        with pytest.raises(ValueError, match=OUT_MESSAGE):
            _operands.result_array((3, 5), np.uint16, True, 0, out)
    bad_host = {"shape": np.zeros((3, 6), np.uint16), "dtype": np.zeros((3, 5), np.float32), "strided": np.zeros((3, 6), np.uint16)[:, 1:], "kind": mine}
    for out in bad_host.values():
        with pytest.raises(ValueError, match="out must be a contiguous numpy array of the result shape and dtype"):
            _operands.result_array((3, 5), np.uint16, False, 0, out)


def test_written_bumps_the_version_of_a_library_owned_allocation_only(lib):
    owned = DeviceArray.empty((3, 5), np.float32, 0)
    assert owned._buf.version == 0
    assert _operands.written(owned) is owned and owned._buf.version == 1
    assert _operands.written(owned[1:]) is not None and owned._buf.version == 2      # a window tells its owner
    foreign = settled()
    assert _operands.written(foreign) is foreign                                   # foreign memory has no version: nothing happens
    host = np.zeros(3)
    assert _operands.written(host) is host and _operands.written(None) is None


# ---- the table: every wrapper that accepts a DeviceArray waits for its upload before its entry point ------------------------------------
EYE, ZERO = np.eye(3), np.zeros(3)
RANGES = (0.0, 1.0, 0.0, 1.0)


def _f32(ticket):
    return pending(ticket, address=0x1000 * ticket)


WRAPPERS = {
    "rescale_intensity": ("mvs_rescale_intensity", 1, lambda a: _reg_ops.rescale_intensity(a[0], out_on_device=True)),
    "phase_cross_correlation": ("mvs_phasecorr", 2, lambda a: _reg_ops.phase_cross_correlation(*a)),
    "phase_cross_correlation_multi": ("mvs_phasecorr_multi", 2, lambda a: _reg_ops.phase_cross_correlation_multi(*a)),
    "phase_cross_correlation_multi_refined": ("mvs_phasecorr_multi_refined", 2,
                                              lambda a: _reg_ops.phase_cross_correlation_multi(*a, upsample_factor=4, return_refined=True)),
    "register_crops": ("mvs_register_crops", 2, lambda a: _reg_ops.register_crops(*a, 1)),
    "register_views": ("mvs_register_views", 2, lambda a: _reg_ops.register_views(a[0], [1.0] * 3, [0.0] * 3, a[1], [1.0] * 3, [0.5] * 3, SHAPE, 1)),
    "score_candidates": ("mvs_score_candidates", 2, lambda a: _reg_ops.score_candidates(*a, [[0.0] * 3], "union", 1.0, 0.0)),
    "score_candidates_argmax": ("mvs_score_candidates_argmax", 2, lambda a: _reg_ops.score_candidates_argmax(*a, [[0.0] * 3], "union", 1.0, 0.0, 1.0)),
    "finite_range": ("mvs_finite_range", 1, lambda a: _reg_ops.finite_range(a[0])),
    "affine_normal_equations": ("mvs_affine_normal_eq", 2, lambda a: _reg_ops.affine_normal_equations(*a, EYE, ZERO)),
    "affine_joint_hist": ("mvs_affine_joint_hist", 2, lambda a: _reg_ops.affine_joint_hist(*a, EYE, ZERO, 8, RANGES)),
    "affine_mi_gradient": ("mvs_affine_mi_gradient", 2, lambda a: _reg_ops.affine_mi_gradient(*a, EYE, ZERO, 8, RANGES, np.zeros((8, 8)))),
    "resample_array": ("mvs_resample", 1, lambda a: transformation.resample_array(a[0], EYE, ZERO, SHAPE)),
    "log_response": ("mvs_log_response", 1, lambda a: _detect_ops.log_response(a[0], (1.0, 1.0, 1.0), 1.0)),
    "local_maxima": ("mvs_local_maxima", 2, lambda a: _detect_ops.local_maxima(a[0], (3, 3, 3), 0.0, sample=a[1], sample_window=(3, 3, 3), bound=1.0)),
    "label_components": ("mvs_label_components", 1, lambda a: _label_ops.label_components(a[0], 0.5)),
}


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_a_float32_wrapper_waits_for_its_pending_inputs_first(lib, name):
    entry, n_arrays, call = WRAPPERS[name]
    call([_f32(t) for t in range(1, n_arrays + 1)])
    assert lib.names().count(entry) == 1
    assert sorted(lib.waited_before(entry)) == [(0, t) for t in range(1, n_arrays + 1)]


def test_the_point_set_wrappers_wait_first(lib):
    ref, query = pending(1, (10, 3), np.float64), pending(2, (7, 3), np.float64, address=0x2000)
    idx, dist = _marker_ops.knn(ref, query, 2)
    assert idx.shape == dist.shape == (7, 2) and sorted(lib.waited_before("mvs_knn")) == [(0, 1), (0, 2)]
    _marker_ops.descriptors(pending(3, (10, 3), np.float64), np.zeros((10, 4), np.int32), 3, 1)
    assert lib.waited_before("mvs_marker_descriptors")[-1] == (0, 3)
    for bad in (settled((10, 3), np.float32), settled((10, 4), np.float64)[:, 1:]):
        with pytest.raises(TypeError, match="knn"):
            _marker_ops.knn(bad, bad, 2)
    with pytest.raises(ValueError, match=r"\(n, dim\)"):
        _marker_ops.knn(np.zeros(5), np.zeros(5), 2)


def test_masked_corr_waits_for_crops_and_masks_first(lib):
    crops = [_f32(1), _f32(2)]
    masks = [pending(3, dtype=np.uint8, address=0x3000), pending(4, dtype=np.uint8, address=0x4000)]
    _masked_corr_ops.masked_corr(*crops, *masks, shifts=2)
    assert sorted(lib.waited_before("mvs_masked_corr")) == [(0, 1), (0, 2), (0, 3), (0, 4)]
    host = np.zeros(SHAPE, np.float32)
    with pytest.raises(TypeError, match="both crops must live on the same side"):
        _masked_corr_ops.masked_corr(crops[0], host, shifts=2)
    with pytest.raises(TypeError, match="both masks must live on the same side"):
        _masked_corr_ops.masked_corr(host, host, masks[0], host > 0, shifts=2)
    with pytest.raises(TypeError, match="uint8"):
        _masked_corr_ops.masked_corr(host, host, _f32(5), None, shifts=2)


def test_masked_corr_turns_host_masks_into_uint8_and_takes_one_alone(lib):
    host = np.zeros(SHAPE, np.float32)
    _masked_corr_ops.masked_corr(host, host, None, np.full(SHAPE, 2.5), shifts=2)
    (args,) = [a for n, a in lib.calls if n == "mvs_masked_corr"]
    opts = args[6]._obj
    assert args[3] is None and args[4] is not None and (opts.mem, opts.mask_mem) == (_lib.MVS_MEM_HOST, _lib.MVS_MEM_HOST)
    lib.calls.clear()
    _masked_corr_ops.masked_corr(_f32(1), _f32(2), None, None, shifts=2)
    (args,) = [a for n, a in lib.calls if n == "mvs_masked_corr"]
    assert (args[6]._obj.mem, args[6]._obj.mask_mem) == (_lib.MVS_MEM_DEVICE, _lib.MVS_MEM_HOST)


def test_label_contacts_and_apply_plane_wait_first(lib):
    _mask_ops.label_contacts(pending(1, dtype=np.int32), 5)
    assert lib.waited_before("mvs_label_contacts") == [(0, 1)]
    with pytest.raises(TypeError, match="contiguous"):
        _mask_ops.label_contacts(settled((4, 6, 9), np.int32)[:, :, 1:], 5)
    _shading_ops.apply_plane(np.zeros(SHAPE, np.uint16), pending(2, (6, 8, 2)))
    assert lib.waited_before("mvs_plane_apply")[-1] == (0, 2)
    with pytest.raises(ValueError, match="contiguous"):
        _shading_ops.apply_plane(np.zeros(SHAPE, np.uint16), settled((6, 8, 3))[:, :, 1:])


def test_the_result_frames_mark_their_device_results_as_written(lib):
    out = _reg_ops.rescale_intensity(settled(), out_on_device=True)[0]
    assert isinstance(out, DeviceArray) and out._buf.version == 1
    out = transformation.resample_array(settled(), EYE, ZERO, (2, 3, 4))
    assert isinstance(out, DeviceArray) and out.shape == (2, 3, 4) and out.dtype == np.float32 and out._buf.version == 1
    assert isinstance(transformation.resample_array(np.zeros(SHAPE, np.uint16), EYE, ZERO, (2, 3, 4)), np.ndarray)


# ---- strided views: label_view and register_views on view_data / fill_view_geometry ----------------------------------------------------------
def _fields(view, base=0):
    return {"data": view.data - base, "dtype": view.dtype, "mem": view.mem, "shape": list(view.shape), "stride": list(view.stride),
            "matrix": list(view.matrix), "offset": list(view.offset)}


IDENTITY9 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def test_label_view_fills_the_view_as_before(lib):
    """The expected fields are those the function gave before it was built on ``view_data`` / ``fill_view_geometry``."""
    h2 = np.arange(35, dtype=np.int32).reshape(5, 7)
    view, keep = _label_ops.label_view(h2, None, None, 0)
    assert keep is h2 and _fields(view, h2.ctypes.data) == {"data": 0, "dtype": 0, "mem": 0, "shape": [1, 5, 7], "stride": [35, 7, 1],
                                                           "matrix": IDENTITY9, "offset": [0.0, 0.0, 0.0]}
    h3 = np.arange(72, dtype=np.int32).reshape(3, 4, 6)
    view, keep = _label_ops.label_view(h3, [[1, 0, 0], [0, 1, 0.5], [0, 0, 2]], [0.5, -1, 2], 0)
    assert keep is h3 and _fields(view, h3.ctypes.data) == {"data": 0, "dtype": 0, "mem": 0, "shape": [3, 4, 6], "stride": [24, 6, 1],
                                                           "matrix": [1.0, 0.0, 0.0, 0.0, 1.0, 0.5, 0.0, 0.0, 2.0], "offset": [0.5, -1.0, 2.0]}
    window = DeviceArray.from_pointer(0x1000, (4, 6, 8), np.int32, 0)[1:, 2:, 3:]
    view, keep = _label_ops.label_view(window, np.diag([1.0, 2.0, 0.5]), [1.0, 2.0, 3.0], 0)
    assert keep is window and _fields(view) == {"data": 4364, "dtype": 0, "mem": 1, "shape": [3, 4, 5], "stride": [48, 8, 1],
                                                "matrix": [1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.5], "offset": [1.0, 2.0, 3.0]}
    window2 = DeviceArray.from_pointer(0x2000, (6, 8), np.int32, 0)[2:, 3:]
    view, keep = _label_ops.label_view(window2, None, [0.25, -0.75], 0)
    assert keep is window2 and _fields(view) == {"data": 8268, "dtype": 0, "mem": 1, "shape": [1, 4, 5], "stride": [32, 8, 1],
                                                 "matrix": IDENTITY9, "offset": [0.0, 0.25, -0.75]}
    # an x axis of one voxel, whose stride is arbitrary (7 here): the view says 1
    thin = DeviceArray(None, 0x3000, (3, 5, 1), (40, 8, 7), np.int32, 0)
    view, keep = _label_ops.label_view(thin, None, None, 0)
    assert keep is thin and _fields(view) == {"data": 12288, "dtype": 0, "mem": 1, "shape": [3, 5, 1], "stride": [40, 8, 1],
                                              "matrix": IDENTITY9, "offset": [0.0, 0.0, 0.0]}
    thin2 = DeviceArray(None, 0x3000, (5, 1), (8, 7), np.int32, 0)
    view, keep = _label_ops.label_view(thin2, None, None, 0)
    assert keep is thin2 and _fields(view) == {"data": 12288, "dtype": 0, "mem": 1, "shape": [1, 5, 1], "stride": [40, 8, 1],
                                               "matrix": IDENTITY9, "offset": [0.0, 0.0, 0.0]}
    assert lib.calls == []
    view, _ = _label_ops.label_view(pending(6, dtype=np.int32), None, None, 2 << 8)
    assert [(n, a[:2]) for n, a in lib.calls] == [("mvs_event_wait", (2 << 8, 6))]


def test_register_views_fills_both_views_from_strided_slabs(lib):
    slabs = [DeviceArray.from_pointer(0x1000, (4, 6, 8), np.uint16, 0)[1:, 2:, 3:], DeviceArray.from_pointer(0x9000, (6, 8), np.float32, 0)[2:, 3:]]
    _reg_ops.register_views(slabs[0], [1.0, 2.0, 0.5], [1.0, 2.0, 3.0], slabs[0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0], (3, 4, 5), 1)
    args = lib.calls[-1][1]
    assert lib.calls[-1][0] == "mvs_register_views"
    assert _fields(args[1]._obj) == {"data": 0x1000 + 2 * 67, "dtype": _lib.MVS_U16, "mem": 1, "shape": [3, 4, 5], "stride": [48, 8, 1],
                                     "matrix": [1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.5], "offset": [1.0, 2.0, 3.0]}
    assert _fields(args[2]._obj)["matrix"] == IDENTITY9
    _reg_ops.register_views(slabs[1], [2.0, 0.5], [0.25, -0.75], slabs[1], [1.0, 1.0], [0.0, 0.0], (4, 5), 1)
    args = lib.calls[-1][1]
    assert _fields(args[1]._obj) == {"data": 0x9000 + 4 * 19, "dtype": _lib.MVS_F32, "mem": 1, "shape": [1, 4, 5], "stride": [32, 8, 1],
                                     "matrix": [1.0, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.5], "offset": [0.0, 0.25, -0.75]}
    with pytest.raises(TypeError, match="register_views"):
        _reg_ops.register_views(np.zeros(SHAPE, np.float32), [1.0] * 3, [0.0] * 3, slabs[0], [1.0] * 3, [0.0] * 3, SHAPE, 1)
