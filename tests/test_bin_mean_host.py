"""CPU: the arithmetic of every binning kernel (csrc/mvs_bin_dev.h, mvs_bin::mean_cast) compiled for the host.  A block whose sum is
an exact multiple of its count must give exactly that mean -- ``sum * (1.0 / count)`` followed by the truncating cast gives one less
at 505 of the counts up to 4096, first at 49 -- and every other sum must give Python's integer quotient."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_mean_is_exact_for_multiples_and_floors_the_rest(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "bin_mean_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "bin_mean_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    # exact multiples: all 65536 means for the counts 1..4096 and 32768, every 61st (1075 of them) for the 28671 counts between
    n16 = 4096 * 65536 + (32767 - 4096) * 1075 + 65536
    want = {("u16", "u32"): n16, ("u16", "f64"): n16, ("u8", "u32"): 512 * 256, ("u8", "f64"): 512 * 256}
    rows = [ln.split()[1:] for ln in lines if ln.startswith("X ")]
    assert sorted((t, a) for t, a, *_ in rows) == sorted(want)
    for t, a, checked, wrong, count, mean, got in rows:
        print(f"exact multiples {t} (accumulator {a}): {checked} checked, {wrong} wrong")
        assert int(checked) == want[(t, a)]
        assert int(wrong) == 0, f"{t}/{a}: {wrong} of {checked} wrong, first: sum {int(mean) * int(count)} / count {count} -> {got}, not {mean}"

    # every other sum: the integer quotient
    for t, n_max in (("u16", 65535 * 32768), ("u8", 255 * 512)):
        sample = np.array([[int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith(f"N {t} ")], dtype=np.int64)
        assert sample.shape == (20000, 3) and sample[:, 0].max() <= n_max
        assert np.all(sample[:, 0] % sample[:, 1] != 0)
        np.testing.assert_array_equal(sample[:, 2], sample[:, 0] // sample[:, 1])

    # float32 output: one division in double, one rounding to float32 (what numpy's mean(dtype=float64).astype(float32) does)
    f = [ln.split()[1:] for ln in lines if ln.startswith("F ")]
    assert len(f) == 2000
    for s, count, got in f:
        assert np.float32(float(got)) == np.float32(float(s) / int(count)), (s, count, got)
