"""Marker-based registration of one pair, stage by stage: the device path (mvs_knn, mvs_marker_descriptors, mvs_marker_score
through _marker_reg) against the same stages of the numpy / scipy restatement of the reference (tests/marker_oracle.py: cKDTree,
Python loops) on the host, for N beads per view in 3D with default parameters.

Stages: neighbour scale (k = 2 of both sets), descriptors (both sets), matching (descriptor kNN, ratio test, de-duplication),
RANSAC scoring (the hypotheses of 1000 samples against all candidates; the fits are not timed on either side) and one ICP
iteration (transform, k = 1 query, fit).  Every figure is the wall time of the SECOND of two calls (the first warms code
objects, allocator pools and caches), host clock around calls that wait for their result.  The scene is the tests': a
rotation of 0.15 rad plus a shift, noise 0.1, 20 % dropped, 10 % outliers, at the bead density of 200 beads in 200^3.

    python tools/marker_probe.py [--sizes 1000 5000 20000] [--out profiles/marker_registration.txt] [--limit 900]
"""
import argparse
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def second_call(fn):
    fn()
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def probe(n, device):
    from multiview_stitcher_amd import _marker_ops as ops
    from multiview_stitcher_amd import _marker_reg as mr
    from tests import marker_oracle as mo

    nn, red, ratio, max_error = 3, 1, 3.0, 5.0
    fixed, moving, _ = mo.make_pair(3, n, seed=n, box=200.0 * (n / 200.0) ** (1.0 / 3.0), n_outliers=n // 10)
    rows = {}
    # -- device
    fdev, mdev = ops.to_device(fixed, device), ops.to_device(moving, device)
    rows["neighbour scale"] = [second_call(lambda: mr.nearest_neighbor_scale([fdev, mdev], device))]
    scale = rows["neighbour scale"][0][1]
    threshold = float(scale * np.sqrt(6.0))
    rows["descriptors"] = [second_call(lambda: (mr.build_descriptors(fdev, nn, red, device), mr.build_descriptors(mdev, nn, red, device)))]
    (fvec, fidx), (mvec, midx) = rows["descriptors"][0][1]
    rows["matching"] = [second_call(lambda: mr.match_descriptors(fvec, fidx, mvec, midx, ratio, threshold, device))]
    pairs = rows["matching"][0][1]
    fc, mc = fixed[pairs[:, 0]], moving[pairs[:, 1]]
    samples = mr.ransac_samples(len(pairs), 3, 1000, 0)
    affines, valid = mr.fit_transforms_batch(fc[samples], mc[samples], "rigid")
    affines = affines[valid]
    rows["RANSAC scoring"] = [second_call(lambda: ops.score(affines, fc, mc, max_error, device))]
    counts, sums = rows["RANSAC scoring"][0][1]
    best = affines[int(np.argmax(counts))]
    rows["ICP iteration"] = [second_call(lambda: mr.run_icp(fixed, moving, mdev, best, 0.0, "rigid", max_error, 1, 0.0, device))]
    rows["  of which the k = 1 query"] = [second_call(lambda: ops.knn(mdev, mr.transform_pts(fixed, best), 1, device))]
    # -- host
    rows["neighbour scale"].append(second_call(lambda: mo.get_nearest_neighbor_scale(fixed, moving)))
    rows["descriptors"].append(second_call(lambda: (mo.get_descriptors(fixed, nn, red), mo.get_descriptors(moving, nn, red))))
    fdesc, mdesc = rows["descriptors"][1][1]
    rows["matching"].append(second_call(lambda: mo.match_descriptors(fdesc, mdesc, ratio, threshold)))
    host_pairs = rows["matching"][1][1]

    def host_scores():
        out = []
        for a in affines:
            residuals, mask = mo.score_transform(a, fc, mc, max_error)
            out.append((int(mask.sum()), float(residuals[mask].sum())))
        return out

    rows["RANSAC scoring"].append(second_call(host_scores))
    rows["ICP iteration"].append(second_call(lambda: mo.run_icp(fixed, moving, best, 0.0, "rigid", max_error, 1, 0.0)))
    from scipy.spatial import cKDTree

    tree = cKDTree(moving)
    rows["  of which the k = 1 query"].append(second_call(lambda: tree.query(mo.transform_pts(fixed, best), k=1)))
    # the two sides computed the same thing
    same = (abs(scale - rows["neighbour scale"][1][1]) <= 1e-12 * scale and np.array_equal(pairs, host_pairs)
            and [int(c) for c in counts] == [c for c, _ in rows["RANSAC scoring"][1][1]])
    lines = [f"N = {n} beads per view: {fvec.shape[0]} x {mvec.shape[0]} descriptors of length 6, {len(pairs)} candidates, {len(affines)} hypotheses"
             f" (results equal on both sides: {same})"]
    lines.append(f"  {'stage':30s} {'device ms':>12s} {'host ms':>12s} {'host / device':>14s}")
    for name, ((dev_ms, _), (host_ms, _)) in rows.items():
        lines.append(f"  {name:30s} {dev_ms:12.2f} {host_ms:12.2f} {host_ms / dev_ms:14.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 5000, 20000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marker_registration.txt"))
    ap.add_argument("--limit", type=int, default=900, help="seconds after which the probe is ended")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from multiview_stitcher_amd import _lib

    if _lib.device_count() < 1:
        raise SystemExit("marker_probe needs a HIP device")
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(args.limit)
    _lib.init(args.device)
    text = ["Marker-based registration, one pair, 3D, default parameters (tools/marker_probe.py): wall ms of the second of two calls.",
            "device: mvs_knn / mvs_marker_descriptors / mvs_marker_score through _marker_reg, point sets resident;",
            "host: the same stage of tests/marker_oracle.py (cKDTree, Python loops as the reference has them).", ""]
    for n in args.sizes:
        lines = probe(n, args.device)
        print("\n".join(lines), flush=True)
        text += lines + [""]
        with open(args.out, "w") as f:          # (rewritten after every size: a size that hits the limit leaves the others)
            f.write("\n".join(text))
    signal.alarm(0)


if __name__ == "__main__":
    main()
