"""CPU test of what mvs_intensity_apply and mvs_plane_apply share (csrc/mvs_tile_apply.h): the split of a row into a scalar head,
whole vectors and a scalar tail, compiled for the host (tests/native/tile_row_split_host_test.cpp).  A wrong split is a misaligned
16-byte access on the device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_split_is_aligned_and_is_the_rule_the_kernels_spelled_out(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "tile_row_split_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", "tile_row_split_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    lines = r.stdout.strip().splitlines()
    assert lines and lines[-1] == "done", r.stdout[-3000:]
    pairs = {tuple(ln.split()[1:3]): [int(v) for v in ln.split()[3:]] for ln in lines if ln.startswith("T ")}
    assert sorted(pairs) == [("f32", "f32"), ("u16", "f32"), ("u16", "u16"), ("u8", "f32"), ("u8", "u8")]
    for pair, (cases, vectors, order, short_tail, misaligned, forbidden, rule) in pairs.items():
        assert cases == 32 * 32 * 71 * 2 and vectors > cases // 1000, pair         # (vectors: the checks below are not vacuous)
        assert order == 0, f"{pair}: {order} splits out of order"
        assert short_tail == 0, f"{pair}: {short_tail} tails of a vector or more"
        assert misaligned == 0, f"{pair}: {misaligned} misaligned vectors"
        assert forbidden == 0, f"{pair}: {forbidden} vectors where none are allowed"
        assert rule == 0, f"{pair}: {rule} splits differ from the spelled-out rule"
    assert r.returncode == 0
