"""ctypes binding of libmvs_hip.so (C ABI: include/mvs_hip.h).

The library is looked up next to this file (built in-tree by
``__graft_entry__.build()`` / ``csrc/Makefile``).  There is no fallback: if it
cannot be loaded every compute entry point raises ``RuntimeError``.
"""

from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmvs_hip.so")

MVS_U8, MVS_U16, MVS_F32 = 0, 1, 2
MVS_MEM_HOST, MVS_MEM_DEVICE = 0, 1
MVS_FUSE_WEIGHTED_AVERAGE, MVS_FUSE_MAX, MVS_FUSE_SIMPLE_AVERAGE = 0, 1, 2
MVS_WEIGHTS_NONE, MVS_WEIGHTS_CONTENT_BASED = 0, 1
MVS_AFFINE_NEQ_LEN = 12 * 12 + 12 + 7
MVS_AFFINE_MI_GRAD_LEN = 12 + 1
MVS_LOG_MAX_RADIUS = 40
MVS_PAIR_MOMENTS_LEN = 6          # n, mean_f, mean_m, M2_f, M2_m, C_fm
MVS_PAIR_MAX_CANDIDATES = 8
MVS_PAIR_MAX_HALFSPACES = 16
MVS_PAIR_BLOCK_VOXELS = 256
MVS_PAIR_MAX_BLOCKS = 2048
MVS_KNN_MAX_DIM = 15
MVS_KNN_MAX_K = 16
MVS_MARKER_MAX_NEIGHBORS = 5
MVS_PSF_MAX_RADIUS = 31
MVS_INTENSITY_MAX_CELLS = 16
MVS_INTENSITY_MAX_RECORDS = 1024
MVS_INTENSITY_BLOCK_VOXELS = 256
MVS_INTENSITY_MAX_BLOCKS = 1024
MVS_STACK_MAX_VIEWS = 4096
MVS_BLOCKMATCH_MAX_RADIUS = 8
MVS_BLOCKMATCH_MAX_FLOATS = 15360
MVS_BLOCKMATCH_MAX_BLOCKS = 4096
MVS_BLOCKMATCH_MAX_RESULT_BYTES = 64 << 20
MVS_FIELD_MAX_NODES = 16
MVS_STACK_MAX_QUANTILES = 4
MVS_HIST_MAX_BINS = 4096
MVS_MASK_MAX_DILATE = 32
MVS_LABEL_MAX = 2048
MVS_LABEL_COUNT_MAX_CAPACITY = 1 << 31
MVS_LABEL_PAIR_MAX_CAPACITY = 1 << 27
MVS_LABEL_INCOMPLETE = 1        # mvs_label_pair_overlaps: more entries than `capacity` (not an error)
MVS_FEATHER_MAX_WIDTH = 32
MVS_FEATHER_FULL_WEIGHT = 252
MVS_MASKED_CORR_MAX_VOXELS = 1 << 28
MVS_MASKED_CORR_OK, MVS_MASKED_CORR_NO_ELIGIBLE_SHIFT, MVS_MASKED_CORR_TOO_FEW_VALID, MVS_MASKED_CORR_CONSTANT_CROP = 0, 1, 2, 3
MVS_SCORE_COMPLETE, MVS_SCORE_DROPPED, MVS_SCORE_REWALKED = 1, 2, 4      # state_out bits of mvs_score_candidates_argmax
ERR_UNSUPPORTED = -4            # MVS_ERR_UNSUPPORTED

DTYPE_CODES = {np.dtype(np.uint8): MVS_U8, np.dtype(np.uint16): MVS_U16, np.dtype(np.float32): MVS_F32}
CODE_DTYPES = {v: k for k, v in DTYPE_CODES.items()}


class mvs_view_t(C.Structure):
    _fields_ = [
        ("data", C.c_void_p),
        ("dtype", C.c_int32),
        ("mem", C.c_int32),
        ("shape", C.c_int64 * 3),
        ("stride", C.c_int64 * 3),
        ("matrix", C.c_double * 9),
        ("offset", C.c_double * 3),
        ("w_matrix", C.c_double * 9),
        ("w_offset", C.c_double * 3),
        ("edt", C.c_float * 125),
        ("reserved", C.c_int32),
        ("index_offset", C.c_int64 * 3),
    ]


class mvs_fuse_opts_t(C.Structure):
    _fields_ = [
        ("ndim", C.c_int32),
        ("order", C.c_int32),
        ("fusion", C.c_int32),
        ("weights", C.c_int32),
        ("out_shape", C.c_int64 * 3),
        ("trim", C.c_int64 * 3),
        ("sigma_1", C.c_float),
        ("sigma_2", C.c_float),
        ("out_dtype", C.c_int32),
        ("out_mem", C.c_int32),
        ("index_origin", C.c_int64 * 3),
    ]


class mvs_deconv_opts_t(C.Structure):
    _fields_ = [
        ("n_iterations", C.c_int32),
        ("erosion_px", C.c_int32),
        ("lambda_reg", C.c_double),
        ("min_value", C.c_double),
        ("trim", C.c_int64 * 3),
        ("out_dtype", C.c_int32),
        ("flags", C.c_int32),
    ]


MVS_DECONV_PREPARE_WEIGHTS = 1


class mvs_multiband_opts_t(C.Structure):
    _fields_ = [
        ("levels", C.c_int32 * 3),
        ("index_origin", C.c_int64 * 3),
        ("trim", C.c_int64 * 3),
        ("out_dtype", C.c_int32),
        ("flags", C.c_int32),
    ]


MVS_MULTIBAND_MAX_LEVELS = 6
MVS_MULTIBAND_MAX_VIEWS = 254


class mvs_masked_corr_opts_t(C.Structure):
    _fields_ = [
        ("ndim", C.c_int32),
        ("mem", C.c_int32),
        ("mask_mem", C.c_int32),
        ("has_valid_above", C.c_int32 * 2),
        ("reserved", C.c_int32),
        ("valid_above", C.c_double * 2),
        ("overlap_ratio", C.c_double),
        ("min_overlap", C.c_int64),
        ("max_shift", C.c_int64 * 3),
    ]


class mvs_masked_corr_result_t(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("peak", C.c_int32 * 3),
        ("r", C.c_float),
        ("reserved", C.c_int32),
        ("n_peak", C.c_int64),
        ("n_max", C.c_int64),
        ("n_valid", C.c_int64 * 2),
        ("neighbour_r", C.c_float * 6),
        ("neighbour_ok", C.c_int32 * 6),
        ("padded", C.c_int64 * 3),
        ("max_shift", C.c_int64 * 3),
    ]


class mvs_dct_opts_t(C.Structure):
    _fields_ = [
        ("dct_size", C.c_int64 * 3),
        ("output_chunksize", C.c_int64 * 3),
        ("exponent", C.c_double),
        ("otf_support_fraction", C.c_double),
        ("has_otf", C.c_int32),
        ("has_output_chunksize", C.c_int32),
    ]


class mvs_pair_job_t(C.Structure):
    _fields_ = [
        ("fixed", mvs_view_t),
        ("moving", mvs_view_t),
        ("out_shape", C.c_int64 * 3),
        ("wait_ticket", C.c_uint64 * 2),
        ("bin", C.c_int32 * 3),
        ("flags", C.c_int32),
    ]


class mvs_intensity_record_t(C.Structure):
    _fields_ = [
        ("lo", C.c_int64 * 3),
        ("n", C.c_int64 * 3),
        ("cell_f", C.c_int32 * 3),
        ("cell_m", C.c_int32 * 3),
    ]


class mvs_block_t(C.Structure):
    _fields_ = [
        ("lo", C.c_int64 * 3),
        ("n", C.c_int64 * 3),
    ]


# name -> (restype, argtypes); every symbol include/mvs_hip.h declares
SIGNATURES = {
    "mvs_version": (C.c_char_p, []),
    "mvs_device_count": (C.c_int, []),
    "mvs_init": (C.c_int, [C.c_int]),
    "mvs_shutdown": (None, [C.c_int]),
    "mvs_last_error": (C.c_char_p, [C.c_int]),
    "mvs_set_stream": (C.c_int, [C.c_int, C.c_void_p]),
    "mvs_synchronize": (C.c_int, [C.c_int]),
    "mvs_set_option": (C.c_int, [C.c_int, C.c_char_p, C.c_int64]),
    "mvs_get_counter": (C.c_int, [C.c_int, C.c_char_p, C.c_int32, C.POINTER(C.c_double)]),
    "mvs_memcpy_peer": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64]),
    "mvs_last_kernel_ms": (C.c_double, [C.c_int]),
    "mvs_malloc": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "mvs_free": (C.c_int, [C.c_int, C.c_void_p]),
    "mvs_mem_info": (C.c_int, [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "mvs_memcpy_h2d": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mvs_memcpy_d2h": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    "mvs_upload_tile": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]),
    "mvs_memset": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.c_uint64]),
    "mvs_copy_into": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64),
                                C.POINTER(C.c_int64)]),
    "mvs_fuse_chunk": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(mvs_fuse_opts_t), C.c_void_p]),
    "mvs_fuse_chunk_weighted": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.POINTER(mvs_view_t), C.c_int32, C.POINTER(mvs_fuse_opts_t), C.c_void_p]),
    "mvs_resample": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.POINTER(C.c_int64), C.c_int32, C.c_float, C.c_void_p, C.c_int32]),
    "mvs_blend_weights": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_int32]),
    "mvs_blend_weights_at": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p,
                                       C.c_int32]),
    "mvs_fuse_chunk_dct": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(mvs_fuse_opts_t), C.POINTER(mvs_dct_opts_t),
                                     C.c_void_p]),
    "mvs_content_dct_weights": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.POINTER(mvs_dct_opts_t),
                                          C.c_void_p, C.c_void_p, C.c_int32]),
    "mvs_mv_deconv": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64),
         C.c_void_p, C.c_void_p, C.POINTER(mvs_deconv_opts_t), C.c_void_p, C.c_int32],
    ),
    "mvs_multiband_fuse": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.POINTER(mvs_multiband_opts_t), C.c_void_p, C.c_int32],
    ),
    "mvs_phasecorr": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32,
         C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_float)],
    ),
    "mvs_fft_c2c": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32]),
    "mvs_phasecorr_multi": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
         C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_float)],
    ),
    "mvs_phasecorr_multi_refined": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32,
         C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_float), C.c_void_p, C.c_int64],
    ),
    "mvs_rescale_intensity": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float),
         C.POINTER(C.c_int64)],
    ),
    "mvs_bin_mean": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
         C.c_void_p, C.c_int32],
    ),
    "mvs_bin_mean_async": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p],
    ),
    "mvs_bin_mean_batch_async": (
        C.c_int,
        [C.c_int, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
         C.POINTER(C.c_void_p)],
    ),
    "mvs_event_record": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "mvs_event_wait": (C.c_int, [C.c_int, C.c_uint64]),
    "mvs_host_alloc": (C.c_int, [C.c_uint64, C.POINTER(C.c_void_p)]),
    "mvs_host_free": (C.c_int, [C.c_void_p]),
    "mvs_copy_async": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "mvs_mark": (C.c_int, [C.c_int, C.POINTER(C.c_uint64)]),
    "mvs_copy_box": (C.c_int, [C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mvs_ticket_sync": (C.c_int, [C.c_uint64]),
    "mvs_ticket_elapsed_ms": (C.c_int, [C.c_uint64, C.c_uint64, C.POINTER(C.c_double)]),
    "mvs_plan_pairs": (
        C.c_int,
        [C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
         C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64),
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)],
    ),
    "mvs_register_pairs": (
        C.c_int,
        [C.c_int, C.c_int32, C.POINTER(mvs_pair_job_t), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    ),
    "mvs_register_views": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    ),
    "mvs_beads_translation_sweeps": (
        C.c_int,
        [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
         C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)],
    ),
    "mvs_fuse_plan": (
        C.c_int,
        [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
         C.POINTER(C.c_int64), C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)],
    ),
    "mvs_view_graph_prune": (
        C.c_int,
        [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32,
         C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    ),
    "mvs_resolve_translations": (
        C.c_int,
        [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    ),
    "mvs_edge_betweenness": (
        C.c_int,
        [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)],
    ),
    "mvs_register_crops": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
         C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)],
    ),
    "mvs_score_candidates": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double),
         C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.POINTER(C.c_int32)],
    ),
    "mvs_score_candidates_argmax": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double),
         C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32)],
    ),
    "mvs_affine_normal_eq": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.c_double, C.c_double, C.POINTER(C.c_double)],
    ),
    "mvs_affine_joint_hist": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
    ),
    "mvs_affine_mi_gradient": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double),
         C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_double)],
    ),
    "mvs_finite_range": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int64)]),
    "mvs_log_response": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.c_double, C.POINTER(C.c_int64), C.c_void_p, C.POINTER(C.c_float)],
    ),
    "mvs_local_maxima": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_float, C.c_void_p, C.c_int32,
         C.POINTER(C.c_int32), C.c_double, C.POINTER(C.c_int32), C.c_int64, C.POINTER(C.c_int64)],
    ),
    "mvs_pair_moments": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int32,
         C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double)],
    ),
    "mvs_knn": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
         C.POINTER(C.c_double)],
    ),
    "mvs_marker_descriptors": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p, C.c_int32],
    ),
    "mvs_marker_score": (
        C.c_int,
        [C.c_int, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_double,
         C.POINTER(C.c_int32), C.POINTER(C.c_double)],
    ),
    "mvs_psf_extract": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), C.POINTER(C.c_int32),
         C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)],
    ),
    "mvs_intensity_pair_moments": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double),
         C.c_int32, C.POINTER(mvs_intensity_record_t), C.c_int32, C.POINTER(C.c_double)],
    ),
    "mvs_intensity_apply": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32],
    ),
    "mvs_stack_quantiles": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)],
    ),
    "mvs_plane_apply": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32],
    ),
    "mvs_block_match": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.POINTER(mvs_block_t), C.c_int32,
         C.POINTER(C.c_int32), C.POINTER(C.c_double)],
    ),
    "mvs_field_warp": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32],
    ),
    "mvs_tile_histogram": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_double),
         C.POINTER(C.c_double), C.POINTER(C.c_int64)],
    ),
    "mvs_mask_threshold": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_double, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int64)]),
    "mvs_label_fuse": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_int32]),
    "mvs_label_contacts": (C.c_int, [C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]),
    "mvs_label_counts": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    "mvs_label_pair_overlaps": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int64,
         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)],
    ),
    "mvs_label_components": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_float, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(C.c_int64)],
    ),
    "mvs_label_tiles_fuse": (
        C.c_int,
        [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
         C.POINTER(C.c_int64), C.c_void_p, C.c_int32],
    ),
    "mvs_mask_feather": (C.c_int, [C.c_int, C.POINTER(mvs_view_t), C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_int32]),
    "mvs_masked_corr": (
        C.c_int,
        [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(mvs_masked_corr_opts_t),
         C.POINTER(mvs_masked_corr_result_t), C.c_void_p, C.c_void_p],
    ),
}

_lib = None
_lock = threading.Lock()


def load():
    """Load libmvs_hip.so (once). Raises RuntimeError if it is missing/unloadable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libmvs_hip.so not found at {LIB_PATH}: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
                "multiview_stitcher_amd has no CPU fallback."
            )
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


ERR_OUT_OF_MEMORY = -5          # MVS_ERR_OUT_OF_MEMORY (include/mvs_hip.h): a HIP call failed with hipErrorOutOfMemory


class MvsError(RuntimeError):
    """A library call returned a non-zero code; ``code`` is the MVS_ERR_* value of include/mvs_hip.h."""

    def __init__(self, message, code):
        super().__init__(message)
        self.code = int(code)


class DeviceMemoryError(MvsError):
    """MVS_ERR_OUT_OF_MEMORY: the device (or pinned host) allocation of a call did not fit."""


def check(rc, device=0, what="mvs call"):
    if rc != 0:
        msg = load().mvs_last_error(int(device))
        cls = DeviceMemoryError if rc == ERR_OUT_OF_MEMORY else MvsError
        raise cls(f"{what} failed (code {rc}): {msg.decode() if msg else ''}", rc)


def init(device=0):
    lib = load()
    check(lib.mvs_init(int(device)), device, "mvs_init")
    return lib


def device_count():
    return int(load().mvs_device_count())


def i64x3(vals):
    return (C.c_int64 * 3)(*[int(v) for v in vals])


def i32x3(vals, ndim, fill):      # ``fill`` along the z that a 2-D call lacks
    vals = [int(v) for v in vals]
    if len(vals) != ndim:
        raise ValueError(f"expected {ndim} values, got {len(vals)}")
    return (C.c_int32 * 3)(*([fill] * (3 - ndim) + vals))


def synchronize(device=0):
    """Block until all work queued on the context's stream has finished (mvs_synchronize)."""
    check(init(device).mvs_synchronize(int(device)), device, "mvs_synchronize")


def mem_info(device=0):
    """(free, total) bytes of the GPU behind ``device`` (free includes this context's allocation cache)."""
    f, t = C.c_uint64(0), C.c_uint64(0)
    check(init(device).mvs_mem_info(int(device), C.byref(f), C.byref(t)), device, "mvs_mem_info")
    return int(f.value), int(t.value)


def last_kernel_ms(device=0):
    return float(load().mvs_last_kernel_ms(int(device)))


class DeviceBuffer:
    """A device allocation owned by the library (mvs_malloc / mvs_free)."""

    def __init__(self, device, nbytes):
        lib = init(device)
        self.device = int(device)
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib.mvs_malloc(self.device, self.nbytes, C.byref(p)), device, "mvs_malloc")
        self.ptr = p.value
        self.version = 0           # bumped by every write into the allocation: peer copies on other GPUs are stamped with it

    def mark_written(self):
        self.version += 1

    def upload(self, host: np.ndarray):
        host = np.ascontiguousarray(host)
        assert host.nbytes <= self.nbytes
        check(load().mvs_memcpy_h2d(self.device, self.ptr, host.ctypes.data, host.nbytes), self.device, "h2d")
        self.mark_written()
        return self

    def download(self, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(load().mvs_memcpy_d2h(self.device, out.ctypes.data, self.ptr, out.nbytes), self.device, "d2h")
        return out

    def free(self):
        if self.ptr:
            load().mvs_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):  # pragma: no cover
        try:
            self.free()
        except Exception:
            pass


def get_counter(key, device=0, reset=False):
    """mvs_get_counter: a measurement counter of context ``device`` (see include/mvs_hip.h)."""
    v = C.c_double()
    check(init(device).mvs_get_counter(int(device), key.encode(), 1 if reset else 0, C.byref(v)), device, "mvs_get_counter")
    return float(v.value)


def set_option(key, value, device=0):
    check(init(device).mvs_set_option(int(device), key.encode(), int(value)), device, "mvs_set_option")
