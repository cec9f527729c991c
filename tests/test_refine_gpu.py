"""GPU: the upsampled-DFT refinement of the phase correlation (updft_x_kernel, updft_x2_kernel<4>, updft_yx2_kernel<3>,
updft_mid_kernel of csrc/mvs_reg.hip, on the cross power each route leaves them) against the float64 reference of
tests/refine_oracle.py, on pairs with FRACTIONAL shifts (tests/refine_cases.py; tests/test_refine_cases_host.py checks the table on the
CPU).  The refinement's maximum lies off the centre of its window on every pair, and the whole array is read back through
mvs_phasecorr_multi_refined: a kernel row applied for another, a dropped column slot or row, a wrong fold of the y chunks or a wrong
conjugation shows in the array whether or not it moves the maximum."""
import ctypes as C

import numpy as np
import pytest

from oracle import reg_oracle as ro
from tests import refine_oracle
from tests.helpers import _pair_fractional, same_bits
from tests.refine_cases import CASES

pytestmark = pytest.mark.gpu

# max |refined - r64| / max |r64| may not exceed this: a round figure below four times the largest value measured over all cases and
# forms (4.14e-7, see test_refined_array_matches_the_float64_reference), and far below the 1e-5 it may never exceed -- a tenth of the
# smallest refinement gap tests/test_refine_cases_host.py holds the table to, so that an array within the bound has the reference's
# maximum
ARRAY_BOUND = 1.5e-6
assert ARRAY_BOUND <= 1e-5

_inputs, _device = {}, {}


def reference(name):
    """(a, b, {normalisation: (float64 refinement, float32 oracle's shift, its integer peak, float32 restatement's array error)}),
    computed once per case."""
    if name not in _inputs:
        case = CASES[name]
        a, b = _pair_fractional(case.shape, case.true_shift)
        per_norm = {}
        for norm in dict.fromkeys(case.norms):
            r64 = refine_oracle.refinement(a, b, case.upsample, norm, np.float64)
            r32 = refine_oracle.refinement(a, b, case.upsample, norm, np.float32)
            want, wdbg = ro.phase_cross_correlation(a, b, upsample_factor=case.upsample, normalization=norm, return_debug=True)
            per_norm[norm] = (r64, want, wdbg["peak_index"], array_error(r32.refined, r64))
        _inputs[name] = (a, b, per_norm)
    return _inputs[name]


def array_error(refined, r64):
    return float(np.abs(refined.astype(np.complex128) - r64.refined).max() / np.abs(r64.refined).max())


def run_device(name):
    """The case through mvs_phasecorr_multi_refined with the context's options as they stand."""
    from multiview_stitcher_amd import _reg_ops

    case = CASES[name]
    a, b, _ = reference(name)
    return _reg_ops.phase_cross_correlation_multi(a, b, upsample_factor=case.upsample, normalizations=case.norms, return_refined=True)


def default_run(name):
    from multiview_stitcher_amd import _lib

    if name not in _device:
        _lib.get_counter("reg_slab_pairs", reset=True)
        got = run_device(name)
        _device[name] = (got, _lib.get_counter("reg_slab_pairs", reset=True))
    return _device[name]


def check_array(name, got, label=""):
    case = CASES[name]
    _, _, per_norm = reference(name)
    U = int(np.ceil(1.5 * case.upsample))
    for (_, dbg), norm in zip(got, case.norms):
        r64, _, want_peak, err32 = per_norm[norm]
        np.testing.assert_array_equal(dbg["peak_index"], want_peak)      # the device refines the reference's window
        refined = dbg["refined"]
        assert refined.dtype == np.complex64 and refined.shape == (U,) * len(case.shape)
        err = array_error(refined, r64)
        print(f"{name} {label} {norm}: array error {err:.2e} (float32 restatement {err32:.2e}), refinement gap {r64.refined_gap:.2e}")
        assert err <= ARRAY_BOUND, (name, label, norm, err)


def check_shift(name, got):
    case = CASES[name]
    _, _, per_norm = reference(name)
    for (shift, dbg), norm in zip(got, case.norms):
        _, want, want_peak, _ = per_norm[norm]
        np.testing.assert_array_equal(dbg["peak_index"], want_peak)
        assert shift.dtype == np.float32 and want.dtype == np.float32
        assert same_bits(shift, want), (name, norm, shift, want)
        np.testing.assert_array_equal(shift, np.array(case.shift[norm], dtype=np.float32))


@pytest.mark.parametrize("name", sorted(CASES))
def test_refined_array_matches_the_float64_reference(hip_device, name):
    """The refinement array of every case and normalisation against the float64 reference, after the integer peak: max |refined - r64|
    / max |r64| <= ARRAY_BOUND.  The kernels add per lane and then across lanes, numpy's matrix product in another order: both round
    like float32, neither is the other bit for bit.

    Measured on the MI355X, default form, "phase" then None; in brackets the float32 restatement of the reference (complex64 transforms
    and kernels in numpy) on the same pair:
        slab                         5.5e-08 (7.5e-08)   1.7e-07 (1.5e-07)
        merged_peaks_from_last_pass  2.2e-07 (1.7e-07)   2.0e-07 (1.4e-07)
        merged_moves_on_three_axes   7.7e-08 (3.1e-07)   2.1e-07 (2.1e-07)
        merged_nx20                  2.3e-07 (3.5e-07)   1.6e-07 (1.2e-07)
        merged_3_chunks              1.2e-07 (1.9e-07)   1.7e-07 (1.9e-07)
        merged_2_chunks_nx100        1.1e-07 (3.1e-07)   3.3e-07 (1.7e-07)
        merged_2_chunks_nx256        1.3e-07 (1.2e-07)   3.2e-07 (1.9e-07)
        merged_workload              8.6e-08 (1.4e-07)   1.6e-07 (2.6e-07)
        fused_xp_3d                  3.2e-07 (2.5e-07)   1.2e-07 (1.7e-07)
        fused_xp_2d                  9.1e-08 (1.4e-07)   7.9e-08 (1.1e-07)
        fused_xp_2d_bluestein        9.5e-08 (2.2e-07)   4.4e-08 (1.6e-07)
        packed_unfused_3d            1.7e-07 (1.6e-07)   2.5e-07 (1.5e-07)
        packed_unfused_2d_nx300      7.9e-08 (5.4e-07)   1.0e-07 (3.5e-07)
        per_norm_phase_twice         1.9e-07 (2.2e-07)
        single_normalisation                             1.9e-07 (1.1e-07)
        factor10_2d                  1.6e-07 (2.1e-07)   2.7e-07 (2.8e-07)
        factor10_2d_primes           8.7e-08 (5.3e-07)   2.8e-07 (4.7e-07)
        factor3_2d                   1.1e-07 (2.4e-07)   5.9e-08 (1.8e-07)
        factor10_3d                  1.3e-07 (3.7e-07)   1.7e-07 (4.8e-07)
        unit_axis_3d                 1.1e-07 (2.7e-07)   1.3e-07 (3.9e-07)
    Largest per option of test_every_form_matches_the_reference: reg_unfused, materialize_shifts, fft_no_pair 3.2e-07, fft_no_slab
    1.7e-07, fft_no_line 4.1e-07 (merged_nx20, "phase").  The device is as close to float64 as numpy's float32 is: nothing to explain."""
    got, slab_pairs = default_run(name)
    assert slab_pairs == (1.0 if CASES[name].route == "slab" else 0.0)
    check_array(name, got)


@pytest.mark.parametrize("name", sorted(CASES))
def test_shift_and_integer_peak_bit_equal_to_the_oracle(hip_device, name):
    """Shift and integer peak of every normalisation equal oracle.reg_oracle.phase_cross_correlation's (float32 images, as the
    reference calls skimage) bit for bit: the table's off-centre shift.  The single-normalisation case also goes through mvs_phasecorr."""
    from multiview_stitcher_amd import _reg_ops

    got, _ = default_run(name)
    check_shift(name, got)
    case = CASES[name]
    if len(case.norms) == 1:
        a, b, per_norm = reference(name)
        shift, dbg = _reg_ops.phase_cross_correlation(a, b, upsample_factor=case.upsample, normalization=case.norms[0], return_debug=True)
        check_shift(name, [(shift, dbg)])
        # the plain entry runs the same launches: the same bits as the one that reads the refinement back
        plain = _reg_ops.phase_cross_correlation_multi(a, b, upsample_factor=case.upsample, normalizations=case.norms)
        assert same_bits(plain[0][0], got[0][0]) and plain[0][1]["peak_abs"] == got[0][1]["peak_abs"] and "refined" not in plain[0][1]


FORMS = [(option, name) for option in ("reg_unfused", "materialize_shifts", "fft_no_slab", "fft_no_pair", "fft_no_line")
         for name in sorted(CASES) if option in CASES[name].forms]


@pytest.mark.parametrize("option,name", FORMS)
def test_every_form_matches_the_reference(hip_device, option, name):
    """Each option of the context on the cases it changes (``forms`` of the table): the separate launches, one inverse transform per
    normalisation, no three-pass form, flat line order in the first inverse pass, Bluestein instead of whole-line transforms -- every
    one against the float64 reference and the oracle's shift, by the bounds of the default form, not against each other."""
    from multiview_stitcher_amd import _lib

    _lib.set_option(option, 1)
    try:
        _lib.get_counter("reg_slab_pairs", reset=True)
        got = run_device(name)
        slab_pairs = _lib.get_counter("reg_slab_pairs", reset=True)
    finally:
        _lib.set_option(option, 0)
    assert slab_pairs == 0.0      # each of the options that change the slab case leaves the three-pass form
    check_array(name, got, option)
    check_shift(name, got)


def test_device_resident_inputs_give_the_same_bits(hip_device):
    from multiview_stitcher_amd import _reg_ops
    from multiview_stitcher_amd.device import DeviceArray

    name = "merged_2_chunks_nx100"
    case = CASES[name]
    a, b, _ = reference(name)
    host, _ = default_run(name)
    dev = _reg_ops.phase_cross_correlation_multi(DeviceArray.from_host(a), DeviceArray.from_host(b), upsample_factor=case.upsample,
                                                 normalizations=case.norms, return_refined=True)
    for (hs, hd), (ds, dd) in zip(host, dev):
        assert same_bits(hd["refined"], dd["refined"]) and same_bits(hs, ds)
        np.testing.assert_array_equal(hd["peak_index"], dd["peak_index"])
        assert hd["peak_abs"] == dd["peak_abs"]


def test_refined_entry_refuses_bad_arguments(hip_device):
    """A capacity one float short and a NULL refined_out with upsample_factor > 1 are MVS_ERR_INVALID_ARG, refused before anything is
    staged or launched (the outputs keep their bits); upsample_factor == 1 writes nothing and takes a NULL; the next call works."""
    from multiview_stitcher_amd import _lib, _reg_ops

    lib = _lib.init(0)
    name = "fused_xp_2d"
    case = CASES[name]
    a, b, _ = reference(name)
    shape = _lib.i64x3((1,) + case.shape)
    norms = (C.c_int32 * 2)(1, 0)
    need = 2 * 2 * 3 * 3

    def call(upsample, refined, capacity):
        shift, peak, pabs = (C.c_double * 6)(*[7.0] * 6), (C.c_int64 * 6)(*[-7] * 6), (C.c_float * 2)(-7.0, -7.0)
        rc = lib.mvs_phasecorr_multi_refined(0, a.ctypes.data, b.ctypes.data, _lib.MVS_MEM_HOST, 2, shape, norms, 2, upsample, shift, peak, pabs,
                                             refined.ctypes.data if refined is not None else None, capacity)
        return rc, list(shift), list(peak), list(pabs)

    sentinel = np.full(need, -7.0, dtype=np.float32)
    for refined, capacity, message in ((sentinel, need - 1, "refined_capacity"), (None, need, "NULL refined_out")):
        rc, shift, peak, pabs = call(2, refined, capacity)
        assert rc == -1                                                       # MVS_ERR_INVALID_ARG
        assert message in lib.mvs_last_error(0).decode()
        assert shift == [7.0] * 6 and peak == [-7] * 6 and pabs == [-7.0] * 2 and np.all(sentinel == -7.0)
    rc, shift, peak, pabs = call(1, None, 0)
    assert rc == 0 and peak[1:3] != [-7, -7]
    rc, shift, peak, pabs = call(1, sentinel, need)
    assert rc == 0 and np.all(sentinel == -7.0)
    assert _reg_ops.phase_cross_correlation_multi(a, b, upsample_factor=1, normalizations=case.norms, return_refined=True)[0][1]["refined"] is None
    rc, shift, peak, pabs = call(2, sentinel, need)                          # exactly enough
    assert rc == 0 and not np.any(sentinel == -7.0)
    got, _ = default_run(name)
    assert same_bits(sentinel.view(np.complex64).reshape(2, 3, 3), np.stack([d["refined"] for _, d in got]))
