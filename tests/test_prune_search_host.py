"""csrc/mvs_prune_search.h on the HOST: the pruned arg-max search of the candidate scoring is plain host arithmetic, so it is
compiled for the CPU and driven by a fake walk -- per candidate one exact (dyadic) per-voxel value per work item, none above
1 + slack -- on seeded and hand-made cases, for 32 and 16 residue classes, on item grids with partial tiles and with fewer items
than classes.  Every case asserts: the arg max of the reported sums is the arg max of the complete sums; every candidate ends
complete or dropped with a bound below the best complete sum; a candidate without a sample above im1_min and a NaN sum never
serve as the reference sum; near ties of the float32 walk are re-walked and decided by the float64 sums; the per-residue volumes
add up to the cropped interior and equal, item by item, what the kernels' own geometry (WalkGeom) walks.  Needs hipcc only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pruned_search_against_complete_sums_on_a_fake_walk(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path / "prune_search_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "prune_search_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    lines = r.stdout.strip().splitlines()
    assert "K 32 hand-made: ok" in lines and "K 16 hand-made: ok" in lines
    last = lines[-1].split()      # "seeded cases N failures F"
    assert int(last[2]) >= 4000 and int(last[4]) == 0
