"""CPU: csrc/mvs_phasecorr_plan.h compiled for the host (tests/native/phasecorr_plan_host_test.cpp) -- what mvs_phasecorr_multi decides
without the device.  The pass rule against the dispatch conditions of mvs_fft3_c2c, the plan against the conditions the driver evaluated
inline before the header existed (both kept in the C++ file as the "before" predicates), the mailbox and scratch layouts, and the host
arithmetic of skimage's phase_cross_correlation against oracle/reg_oracle.py's expressions in numpy float32."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.fft

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    exe = tmp_path_factory.mktemp("phasecorr_plan") / "phasecorr_plan_host_test"
    cmd = [hipcc, "-O1", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "multiview-stitcher_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "phasecorr_plan_host_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    out = r.stdout.strip().splitlines()
    assert out[-1] == "done"
    return out


def _rows(lines, tag):
    return [ln.split()[1:] for ln in lines if ln.startswith(tag + " ")]


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_prediction_equals_dispatch(lines):
    """Every line length 2..4200, fft_no_line x fft_no_pair, 1..70 lines: kernel family, lines per workgroup and grid of the pass rule
    equal the dispatch; the old predictor agrees with the dispatch; the peak capacity holds the last pass's workgroups; fuse_xp is never
    planned where the first inverse pass would not take it; the planned number of peak entries is the pass's grid."""
    (row,) = _rows(lines, "P")
    checked, *wrong = (int(v) for v in row)
    names = ("kind", "lines_per_wg", "grid", "predictor", "capacity", "fuse_xp", "n_peak")
    print("pass sweep:", checked, "cases;", dict(zip(names, wrong)))
    assert checked == 4199 * 4 * 70
    assert dict(zip(names, wrong)) == dict.fromkeys(names, 0)


def test_route_table_equals_the_inline_conditions(lines):
    routes = {name: int(count) for name, count in _rows(lines, "R")}
    stage1 = {name: int(count) for name, count in _rows(lines, "S")}
    forward = {name: int(count) for name, count in _rows(lines, "F")}
    peaks = {name: int(count) for name, count in _rows(lines, "K")}
    for title, table in (("route", routes), ("stage 1", stage1), ("forward transform", forward), ("peak search", peaks)):
        for name, count in table.items():
            print(f"{title} {name}: {count}")
    assert sorted(routes) == sorted(["slab", "packed_fused_yx", "packed_fused_x", "packed_unfused", "per_norm"]) and min(routes.values()) > 0
    assert sorted(stage1) == sorted(["per_norm", "both", "stages_1_and_2_both"]) and min(stage1.values()) > 0
    assert len(forward) == 3 and min(forward.values()) > 0 and len(peaks) == 3 and min(peaks.values()) > 0
    (row,) = _rows(lines, "RW")
    # (14^3 + 14^2 shapes) x (2 + 4 sets of normalisations) x 4 upsample factors x 32 switch combinations x 3 slab-axis masks
    assert int(row[0]) == (14 ** 3 + 14 ** 2) * 6 * 4 * 32 * 3 == sum(routes.values())
    assert int(row[1]) == 0, row


def test_layouts(lines):
    (row,) = _rows(lines, "L")
    assert int(row[0]) == (14 ** 3 + 14 ** 2) * 6 * 4 * 32 * 3
    assert int(row[1]) == 0, row
    (row,) = _rows(lines, "Y")      # ny = 4..4096 on the merged stages 1 and 2
    assert int(row[0]) == 4093 * 9 and int(row[1]) == 0, row


def test_peak_to_shift_rounding_and_offsets_bit_equal(lines):
    rows = _rows(lines, "A")
    assert len(rows) == 6 * 5 * 5
    for n, uf_i, pk, U, s0, s1, off in (tuple(int(v) for v in r) for r in rows):
        # oracle/reg_oracle.py phase_cross_correlation, one axis, float32 like image_product.real.dtype
        shift = np.float32(pk)
        if shift > np.fix(n / 2):
            shift = np.float32(shift - np.float32(n))
        assert _f32(s0) == shift, (n, uf_i, pk)
        uf = np.array(uf_i, dtype=np.float32)
        rounded = np.round(shift * uf) / uf
        size = np.ceil(uf * 1.5)
        dftshift = np.fix(size / 2.0)
        offset = dftshift - rounded * uf
        assert rounded.dtype == np.float32 and offset.dtype == np.float32 and int(size) == U
        assert _f32(s1).tobytes() == np.float32(rounded).tobytes() and _f32(off).tobytes() == np.float32(offset).tobytes(), (n, uf_i, pk)
    # the sub-pixel maximum m on every axis: shift += (m - dftshift) / uf; 2D keeps axis 0 out of it, an axis of length 1 reports 0
    by_key = {(int(r[0]), int(r[1]), int(r[2])): _f32(int(r[5])) for r in rows}
    mrows = _rows(lines, "M")
    assert len(mrows) >= len(rows) * 2
    for n, uf_i, pk, m, *got in (tuple(int(v) for v in r) for r in mrows):
        uf = np.array(uf_i, dtype=np.float32)
        base = by_key[(n, uf_i, pk)]
        dftshift = np.fix(np.ceil(uf * 1.5) / 2.0)
        want = np.float32(base + (np.float32(m) - dftshift) / uf)
        got = _f32(got)
        assert np.array_equal(got[:3], [want] * 3), (n, uf_i, pk, m)
        assert got[3] == 0 and np.array_equal(got[4:], [want] * 2), (n, uf_i, pk, m)


def test_unravel_partial_argmax_and_subpixel_argmax(lines):
    for flat, nz, ny, nx, pz, py, px in (tuple(int(v) for v in r) for r in _rows(lines, "U")):
        assert np.unravel_index(flat, (nz, ny, nx)) == (pz, py, px)
    tp = _rows(lines, "TP")
    assert len(tp) == 5
    ties = 0
    for r in tp:
        n = int(r[0])
        val, idx = np.array(r[1:1 + n], dtype=np.float32), np.array(r[1 + n:1 + 2 * n], dtype=np.int64)
        best, bi = float(r[1 + 2 * n]), int(r[2 + 2 * n])
        if val.max() < 0:      # nothing above the initial -1: index 0 (the kernels never write a negative modulus)
            assert (best, bi) == (-1.0, 0)
            continue
        ties += int((val == val.max()).sum() > 1)
        assert best == val.max() and bi == idx[val == val.max()].min(), r      # the lowest flat index among the equal maxima
    assert ties >= 3
    ts = _rows(lines, "TS")
    assert len(ts) == 4
    for r in ts:
        n = int(r[0])
        z = np.array(r[1:1 + 2 * n], dtype=np.float32).view(np.complex64)
        assert int(r[1 + 2 * n]) == int(np.argmax(np.abs(z))), r
    assert sum(int((np.abs(z) == np.abs(z).max()).sum() > 1) for z in
               (np.array(r[1:-1], dtype=np.float32).view(np.complex64) for r in ts)) >= 3


def test_kernel_vectors_within_one_ulp_of_numpy(lines):
    rows = _rows(lines, "KV")
    assert len(rows) == 4 * 5 * 5
    offs = {(int(r[0]), int(r[1]), int(r[2])): _f32(int(r[6])) for r in _rows(lines, "A")}
    worst = 0.0
    for r in rows:
        n, uf_i, pk, U = (int(v) for v in r[:4])
        got = _f32([int(v) for v in r[4:]]).reshape(U, n, 2)
        # oracle/reg_oracle.py upsampled_dft, evaluated in double (a float32 upsample factor would round 1 / (n uf) to float32 inside
        # fftfreq) and rounded once to complex64
        kernel = (np.arange(U) - offs[(n, uf_i, pk)])[:, None] * scipy.fft.fftfreq(n, float(uf_i))
        want = np.exp(-1j * 2 * np.pi * kernel).astype(np.complex64)
        for g, w in ((got[..., 0], want.real), (got[..., 1], want.imag)):
            ulp = np.spacing(np.maximum(np.abs(g), np.abs(w)).astype(np.float32))
            err = np.abs(g.astype(np.float64) - w.astype(np.float64)) / ulp
            worst = max(worst, float(err.max()))
    print("kernel vectors: largest difference", worst, "float32 ulp")
    assert worst <= 1.0


def test_channel_scales_are_the_powers_of_two_of_the_device_formula(lines):
    rows = _rows(lines, "X")
    assert len(rows) == 4 * 3 * 3
    for re, im, n, sp, sl in (tuple(int(v) for v in r) for r in rows):
        with np.errstate(over="ignore"):
            dc = np.abs(_f32(re) * _f32(im))      # (1e30 * 1e30: inf, the scale stays 1)
        plain = np.float32(2.0) ** -int(np.floor(np.log2(dc))) if 0 < dc < np.inf else np.float32(1)
        phase = np.float32(2.0) ** -int(np.floor(np.log2(np.float32(n))))
        assert _f32(sl) == plain and _f32(sp) == phase, (re, im, n)
