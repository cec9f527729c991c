"""CPU: how the histogram rank kernels divide a crop among their workgroups (csrc/mvs_rank_plan.h) compiled for the host.  The
counting pass keeps 16-bit counters in LDS and a background slab gives every voxel of a workgroup the same key, so the launch
hist_ranks_apply sizes must leave no workgroup more than 65535 voxels of the ranges hist_rank_kernel takes.  Sizing the launch
from n / 4 instead of the kernel's ceil(n / 4) groups gave a workgroup 65536 voxels at n = 4 * 16383 * k + 1..3 for k = 256 and
k >= 2048 (16776193..16776195, 327660001..327660003: 18 of the sizes below)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every n in 1..70000; 4 * 16383 * k + r, r in -4..4, for k in 1..300, 2046..2050, 5000, 30000; 2^31 - 9 (the largest accepted n)
N_CHECKED = 70000 + 9 * (300 + 5 + 2) + 1


def test_histogram_launch_keeps_the_counters_and_tiles_the_groups(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "rank_plan_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "rank_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "done"

    checked, accepted = (int(v) for v in next(ln for ln in lines if ln.startswith("C ")).split()[1:])
    assert checked == N_CHECKED
    assert accepted == checked          # every one of them needs at most 65535 workgroups
    rows = {ln.split()[1]: [int(v) for v in ln.split()[2:]] for ln in lines if ln.startswith("W ")}
    assert sorted(rows) == ["counters", "cover", "fold", "grid", "tiling"]
    for what, (wrong, n, hgb, per) in rows.items():
        print(f"{what}: {wrong} of {checked} sizes wrong")
        assert wrong == 0, f"{what}: {wrong} sizes wrong, first n = {n}: {hgb} workgroups of {per} groups = {4 * per} voxels"
