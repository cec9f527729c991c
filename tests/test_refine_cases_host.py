"""CPU: the table of the sub-pixel refinement tests (tests/refine_cases.py) holds what it claims -- on the float64 reference
(tests/refine_oracle.py) and on csrc/mvs_phasecorr_plan.h compiled for the host -- so that tests/test_refine_gpu.py may ask the device
for the reference's window, the reference's off-centre maximum and the claimed kernels.  These are conditions on the reference and on
host code: a case that misses one is replaced, the condition stays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import reg_oracle as ro
from tests import refine_oracle
from tests.helpers import _pair_fractional
from tests.refine_cases import CASES, OPTION_BITS, plan_argument

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COARSE_GAP = 1e-2      # the integer peak is then the same in float32 (its transforms round at about 1e-6): the device's window is the reference's
REFINED_GAP = 1e-4     # the float32 restatement's array is 0.8e-7 ... 5.4e-7 of max |refined| from the float64 one on these inputs


@pytest.fixture(scope="module")
def references():
    out = {}
    for name, case in CASES.items():
        a, b = _pair_fractional(case.shape, case.true_shift)
        for norm in dict.fromkeys(case.norms):
            out[name, norm] = (a, b, refine_oracle.refinement(a, b, case.upsample, norm, np.float64))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_leaves_margins_and_moves_off_centre(references, name):
    case = CASES[name]
    for norm in dict.fromkeys(case.norms):
        a, b, ref = references[name, norm]
        print(name, norm, "coarse gap %.2e" % ref.coarse_gap, "refinement gap %.2e" % ref.refined_gap, "sub-pixel step", ref.sub_step.tolist())
        assert ref.coarse_gap >= COARSE_GAP
        assert ref.refined_gap >= REFINED_GAP
        U = int(np.ceil(1.5 * case.upsample))
        assert ref.refined.shape == (U,) * len(case.shape) and ref.refined.dtype == np.complex128
        want_sub = case.sub[norm]
        for axis, n in enumerate(case.shape):
            assert (want_sub[axis] is None) == (n == 1)
            if n > 1:
                assert ref.sub_step[axis] == want_sub[axis], (axis, ref.sub_step.tolist())
        assert any(v for v in want_sub), "the maximum lies at the centre of the window"
        # the float32 oracle reports the table's shift, and the float32 restatement agrees with the float64 one on peak and step
        got = ro.phase_cross_correlation(a, b, upsample_factor=case.upsample, normalization=norm)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, np.array(case.shift[norm], dtype=np.float32))
        r32 = refine_oracle.refinement(a, b, case.upsample, norm, np.float32)
        assert r32.refined.dtype == np.complex64
        np.testing.assert_array_equal(r32.peak_index, ref.peak_index)
        free = np.array(case.shape) > 1
        np.testing.assert_array_equal(r32.sub_step[free], ref.sub_step[free])


def test_table_covers_both_directions_on_every_axis_and_a_merged_case_moving_on_all_three():
    seen = set()
    for case in CASES.values():
        for sub in case.sub.values():
            for axis, v in zip(range(3 - len(case.shape), 3), sub):
                if v:
                    seen.add((axis, v > 0))
    assert seen == {(axis, up) for axis in range(3) for up in (False, True)}
    assert any(c.fuse_yx and c.route == "packed" and all(c.sub[n] and all(c.sub[n]) for n in c.norms) for c in CASES.values())
    assert max(int(np.prod(c.shape)) for c in CASES.values()) <= 1_700_000
    assert set().union(*(c.forms for c in CASES.values())) == set(OPTION_BITS)


def _line_length(n):      # mvs_dft_line_length (csrc/mvs_phasecorr_plan.h)
    if n < 17 or n > 64 or n & (n - 1) == 0:
        return False
    for p in range(2, 20):
        while n % p == 0:
            n //= p
    return n == 1


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("refine_cases") / "phasecorr_plan_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "phasecorr_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    args = [plan_argument(case, option) for case in CASES.values() for option in (None, *OPTION_BITS)]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "done" and len(out) == len(args) + 1
    return {ln.split()[1]: ln.split()[2:] for ln in out[:-1]}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_is_the_one_the_table_claims(plans, name):
    case = CASES[name]
    default = plans[plan_argument(case)]
    route, fuse_xp, fuse_yx, yx_chunks, rows_per_chunk = default[0], int(default[1]), int(default[2]), int(default[3]), int(default[4])
    print(name, default)
    assert (route, fuse_xp, fuse_yx, yx_chunks) == (case.route, int(case.fuse_xp), int(case.fuse_yx), case.yx_chunks)
    if fuse_yx:
        assert rows_per_chunk * yx_chunks >= case.shape[1] > rows_per_chunk * (yx_chunks - 1)
    # the forms: the options under which the plan differs -- and those that change the kernels of a transform without a trace in the
    # plan: fft_no_line moves a pass of a whole-line length to the Bluestein kernels, fft_no_pair changes the order of the lines of a
    # first inverse pass that forms the cross power on the power-of-two register kernel (xp_pairs)
    for option in OPTION_BITS:
        differs = plans[plan_argument(case, option)] != default
        if option == "fft_no_line":
            differs = differs or any(_line_length(n) for n in case.shape)
        if option == "fft_no_pair":
            differs = differs or (route == "packed" and fuse_xp == 1 and case.shape[-1] in (64, 128, 256))
        assert differs == (option in case.forms), option
