"""The pairs of the sub-pixel refinement tests: one table for the CPU test of the table itself (tests/test_refine_cases_host.py: the
float64 reference leaves margins on every case, the plan is the one claimed) and for the GPU tests (tests/test_refine_gpu.py).

Every pair comes from ``tests.helpers._pair_fractional(shape, shift)``: a FRACTIONAL true shift, so that the maximum of the
refinement lies off the centre of its window and the samples around it decide the reported shift.

Per case: shape; true shift; upsample factor; normalisations; what ``mvs_phasecorr_plan::plan`` decides by default -- route
("slab" / "packed" / "per_norm"), fuse_xp, fuse_yx, yx_chunks; per normalisation the sub-pixel arg max in upsampling steps from the
window's centre (``sub``; None on an axis of length 1, whose samples are all equal) and the shift the float32 oracle
``oracle.reg_oracle.phase_cross_correlation`` reports (``shift``; float32 of these decimals); ``forms``: the options of the context
under which its plan differs from the default, or the kernels of its transforms do without a trace in the plan (fft_no_line: an axis of
a whole-line length; fft_no_pair: the first inverse pass forms the cross power on the power-of-two register kernel)."""
from collections import namedtuple

Case = namedtuple("Case", "shape true_shift upsample norms route fuse_xp fuse_yx yx_chunks sub shift forms")

PN = ("phase", None)


def _both(sub, shift):
    return {"phase": sub, None: sub}, {"phase": shift, None: shift}


def _case(shape, true_shift, upsample, norms, route, fuse_xp, fuse_yx, yx_chunks, sub, shift, forms):
    if not isinstance(sub, dict):
        sub, shift = _both(sub, shift)
    return Case(shape, true_shift, upsample, norms, route, fuse_xp, fuse_yx, yx_chunks, sub, shift, forms)


CASES = {
    # three-pass form: forward transform, cross power (long_xp_kernel) and inverse in the slab passes, merged stages 1 and 2
    "slab": _case((64, 64, 18), (3.4, -5.4, 1.6), 2, PN, "slab", True, True, 1, (1, -1, -1), (3.5, -5.5, 1.5),
                  ("reg_unfused", "materialize_shifts", "fft_no_slab", "fft_no_line")),
    # merged stages 1 and 2 (updft_yx2_kernel<3>), one y chunk
    "merged_peaks_from_last_pass": _case((18, 6, 64), (-2.4, 1.4, 5.6), 2, PN, "packed", True, True, 1, (-1, 0, -1), (-2.5, 1.0, 5.5),
                                         ("reg_unfused", "materialize_shifts", "fft_no_pair", "fft_no_line")),
    "merged_moves_on_three_axes": _case((130, 6, 64), (7.4, 0.6, -4.4), 2, PN, "packed", True, True, 1, (1, 1, -1), (7.5, 0.5, -4.5),
                                        ("reg_unfused", "materialize_shifts", "fft_no_pair")),
    # nx = 20: one partly filled lane slot; the two normalisations find different maxima
    "merged_nx20": _case((6, 6, 20), (0.6, -1.4, 2.4), 2, PN, "packed", True, True, 1, {"phase": (0, -1, 1), None: (1, 0, 1)},
                         {"phase": (0.0, -1.5, 2.5), None: (0.5, -1.0, 2.5)}, ("reg_unfused", "materialize_shifts", "fft_no_line")),
    # several y chunks with ragged ends: 3 chunks of 44 rows (the last holds 42); 2 of 33 (the last holds 32), nx = 100 fills the second
    # lane slot partly; all four slots; the workload's proportions, 4 chunks
    "merged_3_chunks": _case((5, 130, 40), (1.4, -6.4, 3.6), 2, PN, "packed", True, True, 3, (0, -1, -1), (1.0, -6.5, 3.5),
                             ("reg_unfused", "materialize_shifts", "fft_no_line")),
    "merged_2_chunks_nx100": _case((7, 65, 100), (-1.4, 4.6, 7.4), 2, PN, "packed", True, True, 2, (0, -1, 1), (-1.0, 4.5, 7.5),
                                   ("reg_unfused", "materialize_shifts")),
    "merged_2_chunks_nx256": _case((9, 70, 256), (2.4, -3.6, 9.4), 2, PN, "packed", True, True, 2, (0, 1, 1), (2.0, -3.5, 9.5),
                                   ("reg_unfused", "materialize_shifts", "fft_no_pair")),
    "merged_workload": _case((51, 256, 128), (3.4, -5.4, 4.6), 2, PN, "packed", True, True, 4, (1, -1, -1), (3.5, -5.5, 4.5),
                             ("reg_unfused", "materialize_shifts", "fft_no_pair", "fft_no_line")),
    # fused cross power without the merge (updft_x2_kernel<4>): 3D with ny < 4, 2D, 2D on the Bluestein register pass with nx < 64
    "fused_xp_3d": _case((2, 3, 64), (0.4, -0.4, 5.4), 2, PN, "packed", True, False, 1, (0, 0, 1), (0.0, 0.0, 5.5),
                         ("reg_unfused", "materialize_shifts", "fft_no_pair")),
    "fused_xp_2d": _case((20, 64), (3.4, -6.4), 2, PN, "packed", True, False, 1, (1, -1), (3.5, -6.5),
                         ("reg_unfused", "materialize_shifts", "fft_no_pair", "fft_no_line")),
    "fused_xp_2d_bluestein": _case((40, 33), (2.6, -4.4), 2, PN, "packed", True, False, 1, (-1, -1), (2.5, -4.5),
                                   ("reg_unfused", "materialize_shifts", "fft_no_line")),
    # packed, nothing fused: the x pass runs on the LDS kernel, xpower_packed_kernel stores P1 and P2, updft_x_kernel per normalisation
    "packed_unfused_3d": _case((3, 5, 130), (0.4, 0.6, -9.4), 2, PN, "packed", False, False, 1, (0, 1, -1), (0.0, 0.5, -9.5),
                               ("materialize_shifts",)),
    "packed_unfused_2d_nx300": _case((3, 300), (0.4, 20.4), 2, PN, "packed", False, False, 1, (0, 1), (0.0, 20.5), ("materialize_shifts",)),
    # one inverse transform per normalisation; the second through n_norm = 1 (mvs_phasecorr is that call)
    "per_norm_phase_twice": _case((4, 6, 64), (0.4, 1.4, -7.4), 2, ("phase", "phase"), "per_norm", False, False, 1, (0, 0, -1), (0.0, 1.0, -7.5),
                                  ("reg_unfused",)),
    "single_normalisation": _case((4, 6, 64), (0.4, 1.4, -7.4), 2, (None,), "per_norm", False, False, 1, (0, 0, -1), (0.0, 1.0, -7.5),
                                  ("reg_unfused",)),
    # the production 2D factor 10: U = 15, updft_x_kernel (nx = 104: its x += 64 loop with a ragged end; nx = 411: seven turns)
    "factor10_2d": _case((53, 104), (-4.37, 6.62), 10, PN, "packed", False, False, 1, (-4, -4), (-4.4, 6.6),
                         ("reg_unfused", "materialize_shifts")),
    "factor10_2d_primes": _case((97, 411), (7.24, -11.43), 10, PN, "packed", False, False, 1, (2, -4), (7.2, -11.4),
                                ("reg_unfused", "materialize_shifts")),
    # factor 3 in 2D: U = 5
    "factor3_2d": _case((24, 40), (2.7, -3.3), 3, PN, "packed", False, False, 1, (-1, -1), (8.0 / 3.0, -10.0 / 3.0),
                        ("reg_unfused", "materialize_shifts", "fft_no_line")),
    # 3D at factor 10: nz * U * U = 18000 outputs of stage 2 > 4096 workgroups x 4, updft_mid_kernel strides its grid
    "factor10_3d": _case((80, 20, 24), (5.27, -2.64, 3.38), 10, PN, "packed", False, False, 1, {"phase": (2, 4, 3), None: (3, 4, 3)},
                         {"phase": (5.2, -2.6, 3.3), None: (5.3, -2.6, 3.3)}, ("reg_unfused", "materialize_shifts", "fft_no_line")),
    # a unit axis in 3D (merged stages 1 and 2 over one plane): its kernel is exactly 1, its shift is reported as 0
    "unit_axis_3d": _case((1, 60, 70), (0, 2.4, -3.4), 2, PN, "packed", True, True, 1, (None, 1, -1), (0.0, 2.5, -3.5),
                          ("reg_unfused", "materialize_shifts", "fft_no_line")),
}

OPTION_BITS = {"reg_unfused": 1, "materialize_shifts": 2, "fft_no_slab": 4, "fft_no_line": 8, "fft_no_pair": 16}


def plan_argument(case, option=None):
    """The case as tests/native/phasecorr_plan_host_test.cpp takes it on its command line."""
    shape3 = (1,) * (3 - len(case.shape)) + tuple(case.shape)
    norms = [1 if v == "phase" else 0 for v in case.norms] + [0]
    return ",".join(str(v) for v in (len(case.shape), *shape3, len(case.norms), norms[0], norms[1], case.upsample, OPTION_BITS.get(option, 0)))
