/* mvs_hip.h -- C ABI of libmvs_hip.so: the MI355X (gfx950) register+fuse hot path
 * for multiview-stitcher workflows.
 *
 * Every entry point below replaces (sits directly beneath) one Python call
 * site of the reference; citations are relative to the reference checkout
 * (src/multiview_stitcher/...).  Nothing in these signatures is a torch type:
 * plain pointers, sizes and POD structs, so the library can be bound from
 * ctypes (what this repo ships), cffi, pybind11 or cgo alike.
 *
 * Conventions
 *   - Arrays are C-contiguous along x; axis order is z,y,x.  2D data is passed
 *     as 3D with shape[0] == 1 (the reference drops a singleton z the same way,
 *     registration.py:2414-2464, fusion/_core.py:701-704).
 *   - "matrix"/"offset" follow scipy.ndimage.affine_transform: they map OUTPUT
 *     pixel indices to INPUT pixel coordinates, in_coord = matrix @ out_idx + offset,
 *     and are produced on the host exactly as transformation.py:37-83 does
 *     (double precision, rounded to 10 decimals, near-integer offsets snapped).
 *   - Return value: 0 = ok, negative = error; the message is available from
 *     mvs_last_error(device).  The Python shim raises RuntimeError.
 *   - Threading: one context per device; calls on the same device serialise on
 *     an internal mutex and run on that context's HIP stream; calls on
 *     different devices are fully concurrent.
 *   - Context lanes: a device argument may carry a lane number in bits 8..11
 *     (`device | lane << 8`, lane < 16): every lane is an independent context on the
 *     same GPU (own stream, scratch buffers, allocation pool and lock), so host
 *     threads that work on independent units (image pairs) overlap on the device
 *     instead of serialising on one lock.  Memory allocated through one lane can be
 *     read by the others once the producing call has returned.
 *   - Ownership: the caller owns every pointer it passes for the duration of
 *     the call.  Device allocations made by mvs_malloc / mvs_upload_tile belong
 *     to the library until mvs_free.
 */
#ifndef MVS_HIP_H
#define MVS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_OK 0
#define MVS_ERR_INVALID_ARG (-1)
#define MVS_ERR_HIP (-2)
#define MVS_ERR_NOT_INITIALISED (-3)
#define MVS_ERR_UNSUPPORTED (-4)
/* a HIP call failed with hipErrorOutOfMemory (device or pinned host allocation): the caller may retry with smaller units */
#define MVS_ERR_OUT_OF_MEMORY (-5)

enum mvs_dtype { MVS_U8 = 0, MVS_U16 = 1, MVS_F32 = 2 };
enum mvs_mem { MVS_MEM_HOST = 0, MVS_MEM_DEVICE = 1 };
/* fusion_func: fusion/_core.py:61-94 (weighted_average_fusion, the default),
 * :42-58 (max_fusion), :97-131 (simple_average_fusion) */
enum mvs_fusion { MVS_FUSE_WEIGHTED_AVERAGE = 0, MVS_FUSE_MAX = 1, MVS_FUSE_SIMPLE_AVERAGE = 2 };
/* weights_func: None | weights.content_based (weights.py:22-74) */
enum mvs_weights { MVS_WEIGHTS_NONE = 0, MVS_WEIGHTS_CONTENT_BASED = 1 };

/* One input view slab of one output chunk: what fuse_np receives per view as
 * (sims[i], params[i], full_view_bbs[i])  -- fusion/_core.py:1513-1531, 1621-1646. */
typedef struct mvs_view_t {
    const void* data;      /* slab voxels, host or device pointer (see mem)            */
    int32_t dtype;         /* enum mvs_dtype; all views of one call share one dtype    */
    int32_t mem;           /* enum mvs_mem                                            */
    int64_t shape[3];      /* slab shape z,y,x                                        */
    int64_t stride[3];     /* element strides z,y,x; stride[2] must be 1             */
    double matrix[9];      /* out px -> slab px  (transformation.py:53-83)           */
    double offset[3];
    double w_matrix[9];    /* out px -> coordinates on the 5^ndim blending support grid */
    double w_offset[3];    /*   (weights.py:448-481 through transformation.py:53-83)  */
    float edt[125];        /* support table, (nz,5,5) row-major, nz = 5 (3D) or 1 (2D);
                              distance_transform_edt of weights.py:459-464 cast to f32 */
    int32_t reserved;
    int64_t index_offset[3]; /* index frame (see mvs_fuse_opts_t.index_origin): first pixel of this slab in the pixel grid
                              that `offset` refers to; 0 = `offset` refers to the slab itself (the reference's per-chunk form) */
} mvs_view_t;

typedef struct mvs_fuse_opts_t {
    int32_t ndim;          /* 2 or 3                                                  */
    int32_t order;         /* interpolation_order 0 | 1  (_core.py:1521, 1627)        */
    int32_t fusion;        /* enum mvs_fusion                                         */
    int32_t weights;       /* enum mvs_weights                                        */
    int64_t out_shape[3];  /* chunk shape INCLUDING halo (output_properties["shape"]) */
    int64_t trim[3];       /* trim_overlap_in_pixels per axis (_core.py:1687-1711)    */
    float sigma_1;         /* content_based sigmas (weights.py:26-27)                 */
    float sigma_2;
    int32_t out_dtype;     /* dtype of the result = input dtype (_core.py:1713)       */
    int32_t out_mem;       /* where `out` lives                                       */
    int64_t index_origin[3]; /* INDEX FRAME.  The reference derives matrix / offset / w_offset per chunk from the chunk's and
                              the slab's origins and rounds them to 10 decimals (transformation.py:72-83), so two chunkings of
                              one mosaic differ by ~1e-9 px in the blend weights -- one count on ~1e-5 of the voxels.  A caller
                              that fuses a stack chunk by chunk (fusion.fuse, the multi-GPU shards) may instead derive every
                              view's parameters ONCE, for output index 0 = a common frame origin (the stack's first voxel) and
                              for pixel 0 of the WHOLE view, and pass here the index of this chunk's first voxel (incl. halo)
                              in that frame and in mvs_view_t.index_offset the first pixel of each slab.  The integer parts
                              are then shifted as integers: every voxel gets the same parameters whatever chunk it falls in.
                              All zeros (the default) = the reference's per-chunk form. */
} mvs_fuse_opts_t;

/* ---- context ---------------------------------------------------------------- */
const char* mvs_version(void);
int mvs_device_count(void);
/* Creates the per-device context (stream, events, scratch pool). Idempotent. */
int mvs_init(int device);
void mvs_shutdown(int device);
const char* mvs_last_error(int device);
/* Run this device's work on an externally owned hipStream_t (e.g. torch's
 * current stream) instead of the context's own stream; NULL restores it. */
int mvs_set_stream(int device, void* hip_stream);
int mvs_synchronize(int device);
/* Tuning / test switches. "force_generic" = 1: mvs_fuse_chunk never takes the translation fast
 * path (both paths must agree; tests compare them).  "no_regions" = 1: skip the region kernels (the column kernel fuses
 * instead; tests compare it with the oracle).  "deconv_general" = 1: mvs_mv_deconv
 * convolves through the general direct path even when separable factors are passed (tests compare both paths).  "dct_general" = 1:
 * the DCT quality pass of mvs_fuse_chunk_dct / mvs_content_dct_weights takes its general path (tests compare both paths).
 * "pool_cache_limit_mb": bytes (MiB) mvs_free may keep cached for later mvs_malloc calls
 * (default 32768; 0 = release immediately).  "materialize_shifts" = 1: mvs_score_candidates / mvs_register_crops
 * always write the shifted copies of the moving image (by default finite-only crops evaluate them inside the SSIM z
 * pass; both ways must agree bit for bit) and mvs_phasecorr_multi runs one inverse transform per normalisation (by default
 * two normalisations share one); tests compare the plain and the default paths.  "serial_classes" = 1: the class kernels of
 * the translation fast path of mvs_fuse_chunk run one after the other on the context's stream (default: side by side on
 * side streams, joined before the call's work is considered done).  "fuse_mixed" = 1 (default 0): the copy class and the
 * one- / two-view classes of that path run as ONE launch over a brick list ordered in space across the classes (measured: no
 * faster, 2 % less HBM traffic -- profiles/round5_fuse_mixed.txt; same voxels).  "rows_v1" = 1: the direct-load row-owning kernels
 * (whole output rows per workgroup, mvs_fuse_rows.hip) are tried before the region kernels for every dtype (default: for
 * float32 tiles only, where they reproduce scipy's NaN propagation through zero-weight taps); it must agree with the
 * default path (tests compare both with the oracle).  Unknown keys -- among them the retired "rowlds" and "stream_rows"
 * of rounds 1-2 -- return MVS_ERR_INVALID_ARG.  "ssim_two_pass" = 1: batched SSIM candidates (and the fixed
 * image's window means) go through the separate z and y / x launches instead of the fused z walks (equal to 1e-9).
 * "reg_unfused" = 1: the phase correlation runs its separate launches (pack, cross power, stored correlation + peak search,
 * one refinement stage per normalisation, a min / max pass over the crops) instead of the fused passes at the ends of the two
 * transforms (bit for bit the same peaks and shifts; tests compare).  "fft_no_line" = 1: axes of 17-64 samples with prime factors
 * <= 19 run on the Bluestein kernels instead of the whole-line register transforms (mvs_dft_small.h; equal to float32 rounding).
 * "fft_no_pair" = 1 (environment MVS_FFT_NO_PAIR for new contexts): the first pass of the inverse transform of the phase correlation takes
 * its lines in flat order instead of as partner pairs (kz, ky), (-kz, -ky) (bit for bit the same; the pairs fetch the packed spectrum once).
 * "fft_slab_axes" = mask (bit k = axis k of (z, y, x); default 4; environment MVS_FFT_SLAB_AXES), "fft_no_slab" = 1 (MVS_FFT_NO_SLAB):
 * crops with ONE short axis (17-64 samples, a whole-line length) and two axes of 64 / 128 / 256 samples whose short axis is in the mask
 * run the phase correlation in three passes over HBM instead of six -- two axes per workgroup, the third forward / cross power /
 * inverse in one kernel (mvs_fft_slab.hip); same peaks and shifts, peak heights to float32 rounding (tests compare).  By default only
 * crops whose short axis is the contiguous one take it: inside the 8-lane pair loop the others are not faster for having half the traffic
 * (profiles/round5_fft_slab.txt).
 * "cb_unpaired" = 1: content-based weights filter value and mask lines in separate launches with separate preparation / quotient
 * kernels (rounds 1-3) instead of gauss1d_pair_kernel; "cb_nosplit" = 1: the paired path keeps both quantities in one workgroup
 * on every pass (all three bit for bit equal; tests compare).  "ssim_prune" = 0: mvs_register_crops / mvs_register_views score
 * every candidate completely (default 1: the arg-max search below; the environment variable MVS_SSIM_PRUNE=0 sets the default
 * of every context created afterwards).  The reference keeps only the candidate with the best SSIM and its rank correlation
 * (registration.py:558-565), and the per-voxel SSIM is <= 1, so a candidate whose partial sum plus (1 + slack) per voxel not
 * yet visited is below the sum of a completely scored candidate cannot win: the candidates of a pair are walked in rounds over
 * growing parts of the volume and dropped as soon as that holds (same selected translation, same quality, same status --
 * tests compare both settings and the oracle).  mvs_score_candidates itself always scores in full. */
int mvs_set_option(int device, const char* key, int64_t value);
/* Measurement counters of one context (bench.py): "reg_alg_bytes" = algorithmic HBM bytes of the pairwise registrations
 * since the last reset (28 n per phase-correlation variant + 20 n per scored candidate + 64 n for the rank correlation, n = crop
 * voxels; a candidate the arg-max search stopped counts the fraction of its volume it was scored on; "reg_alg_bytes_full": every
 * scored candidate counted whole, the reference's formulation), "reg_pairs",
 * "reg_candidates" (candidates that entered the scoring), "reg_pruned" (of these, left unfinished), "reg_cand_volumes"
 * (candidate volumes the SSIM passes went through), "reg_slab_pairs" (phase correlations that ran in three passes: crops with one
 * short and two power-of-two axes; option "fft_no_slab" switches that form off), "reg_rank_hist" / "reg_rank_sort16" / "reg_rank_sort32" (Spearman coefficients
 * computed from key histograms, from sorts on the fixed crop's 16-bit integer keys, from sorts on float keys), "fuse_plan_ms" = host time the last mvs_fuse_chunk spent decomposing the chunk
 * (0 when the plan cached for the same geometry was reused), "fuse_region_bricks" = items (bricks) of the last region-kernel launch,
 * the padding items of the "fuse_mixed" list excluded, "fuse_region_forked" = 1 if that launch ran its class kernels on the side
 * streams (4096 items or more and option "serial_classes" off), else 0.  Per class k of the last region-kernel launch (0 one-view rim
 * boxes, 1 NV = 2, 2 NV <= 4, 3 NV <= 8, 4 copy): "fuse_class_in_vox_<k>" (voxels x views of the class's boxes),
 * "fuse_class_out_vox_<k>", and "fuse_class_ms_<k>" = the class kernel's own duration when that launch ran with option
 * "serial_classes" = 1 (-1 otherwise).  "pool_misses" / "pool_miss_bytes" / "pool_releases": hipMalloc calls (and their bytes) that
 * mvs_malloc could not serve from its cache, blocks mvs_free handed back to the runtime.  "fuse_rows_chunks" / "fuse_region_chunks" /
 * "fuse_column_chunks" / "fuse_generic_chunks": chunks of mvs_fuse_chunk by the kernel family that fused them (row kernels, region
 * kernels, column kernel, generic kernel; one count per family a call launched: a chunk that the column kernel gave up on because a
 * column met more than 64 views, and that the generic kernel redid, counts in both; content-based and DCT-weighted chunks count in
 * none; "fuse_weighted_chunks": the chunks of mvs_fuse_chunk_weighted, which count in none of the four).  With option "no_regions" = 1 a weighted-average chunk goes to the column kernel, which by default takes it only when the
 * region planner declines (more than 8 views on a cell, too many cells or regions); tests assert the family they were built for.
 * Content-based chunks that took the bit-faithful passes: "cb_exact_chunks", "cb_exact_large_chunks" (of these, the ones with more than
 * 8 views or a pool beyond 32-bit indices: boxes read from global memory), and their line launches by kernel: "cb_exact_paired_launches"
 * (value and mask in one launch), "cb_exact_lds_launches" / "cb_exact_tap_launches" (separate passes, LDS-staged / tap by tap).
 * reset != 0 clears an accumulating counter after reading. */
int mvs_get_counter(int device, const char* key, int32_t reset, double* value_out);
/* Device time (ms, hipEvent) spent in the kernels of the most recent compute
 * call on this device; blocks until that work has finished. */
double mvs_last_kernel_ms(int device);

/* ---- device memory / tile residency ----------------------------------------- *
 * The reference moves every chunk across PCIe twice (cp.asarray on entry,
 * cp.asnumpy on exit: fusion/_core.py:1584-1587, 1716-1721).  These handles let
 * register() and fuse() share ONE upload per tile. */
/* mvs_malloc / mvs_free go through a caching pool (a pairwise registration allocates a handful of
 * overlap-sized buffers per pair; hipMalloc/hipFree would cost more than its kernels): memory is
 * uninitialised, and a freed block may be handed out again while earlier work on the context's
 * stream is still queued -- which is safe because all work of this library is ordered on that stream. */
int mvs_malloc(int device, uint64_t nbytes, void** dev_ptr);
int mvs_free(int device, void* dev_ptr);
/* Free / total device memory of the GPU behind `device` (hipMemGetInfo + what the allocation cache of this context would
 * give back).  Used by fusion.fuse to size its launch blocks: output + staged view slabs must fit (the reference sizes its
 * work by output_chunksize alone, fusion/_core.py:248-277, because every chunk there is a separate host task). */
int mvs_mem_info(int device, uint64_t* free_bytes, uint64_t* total_bytes);
int mvs_memcpy_h2d(int device, void* dst_dev, const void* src_host, uint64_t nbytes);
int mvs_memcpy_d2h(int device, void* dst_host, const void* src_dev, uint64_t nbytes);
int mvs_upload_tile(int device, const void* host, int32_t dtype, const int64_t shape[3], void** dev_ptr);
/* Copy between two GPUs of the node (peer access over xGMI when available): ordered after the work queued on the
 * source context, returns when the bytes have arrived.  The multi-GPU farms fetch the halo tiles of a pair / chunk
 * owner from the neighbour that holds them with this (reference precedent: browser/executors.py:166-194, 267-281,
 * where every worker re-reads its inputs from storage). */
int mvs_memcpy_peer(int dst_device, void* dst_dev, int src_device, const void* src_dev, uint64_t nbytes);
/* Stream-ordered byte fill of device memory (returns without waiting). */
int mvs_memset(int device, void* dst_dev, int32_t byte_value, uint64_t nbytes);
/* Device-to-device copy of a contiguous (z,y,x) box into a window of a larger contiguous array (both on this
 * device; stream-ordered, returns without waiting): how the chunks of a chunked fuse() are assembled into one
 * device-resident mosaic (the reference's chunks each go to their own zarr region, fusion/_core.py:1123-1141). */
int mvs_copy_into(int device, const void* src_dev, int32_t dtype, const int64_t shape[3],
                  void* dst_dev, const int64_t dst_shape[3], const int64_t dst_offset[3]);
/* Device-to-device copy of a box of box[0] planes x box[1] rows x box[2] BYTES per row between two pitched arrays on this device
 * (pitch[0]: bytes from row to row, pitch[1]: from plane to plane; rows contiguous; stream-ordered, returns without waiting).  A
 * streamed fuse() re-tiles a fused launch block with it so that every Zarr chunk of the block is ONE contiguous piece of the
 * download and goes to its chunk file without a gather on the host (fusion/_core.py:1123-1171 writes regions of a dask array). */
int mvs_copy_box(int device, const void* src_dev, const int64_t src_pitch[2], void* dst_dev, const int64_t dst_pitch[2], const int64_t box[3]);

/* ---- fusion ------------------------------------------------------------------ *
 * mvs_fuse_chunk == the body of fusion.fuse_np (fusion/_core.py:1608-1713) for
 * the built-in fusion_func / weights_func: per view affine resample
 * (transformation.py:136-139 -> scipy.ndimage.affine_transform, cval = NaN),
 * blending weights (weights.py:391-511), mask by ~isnan + normalise
 * (_core.py:1648-1649, weights.py:325-345), optional content-based weights,
 * fusion_func, trim halo, nan_to_num, cast to the input dtype -- as ONE fused
 * kernel (no per-view float32 temporaries).  `out` has shape out_shape - 2*trim. */
int mvs_fuse_chunk(int device, const mvs_view_t* views, int32_t n_views,
                   const mvs_fuse_opts_t* opts, void* out);

/* Single-view resample == transformation.transform_sim's scipy call
 * (transformation.py:136-139) with order 0|1, mode="constant", cval; float32
 * output.  Used for registration's pre-transform (registration.py:318-338) and
 * for fusion with user-supplied fusion_func/weights_func callables.
 * Only matrix/offset/data/shape/stride/dtype/mem of `view` are read. */
int mvs_resample(int device, const mvs_view_t* view, const int64_t out_shape[3],
                 int32_t order, float cval, float* out, int32_t out_mem);

/* Blending-weight volume of one view == weights.get_blending_weights
 * (weights.py:391-511): resampled 5^ndim support + cosine ramp, NOT normalised. */
int mvs_blend_weights(int device, const mvs_view_t* view, int32_t ndim,
                      const int64_t out_shape[3], float* out, int32_t out_mem);
/* The same volume in an INDEX FRAME: w_matrix / w_offset of `view` are derived for the frame's grid, and the volume's first voxel
 * is voxel index_origin (z,y,x; |index_origin| and index_origin + out_shape at most 2^30) of that grid.  The coordinates are formed
 * from the integer sum index + index_origin, so a voxel gets the same bits in any chunk of the frame (mvs_multiband_fuse's
 * chunk-invariant winner map rests on it).  index_origin 0 is mvs_blend_weights. */
int mvs_blend_weights_at(int device, const mvs_view_t* view, int32_t ndim, const int64_t out_shape[3],
                         const int64_t index_origin[3], float* out, int32_t out_mem);

/* ---- DCT-entropy fusion weights ------------------------------------------------ *
 * Options of weights.content_based_dct (weights.py:77-290 of the reference). */
typedef struct mvs_dct_opts_t {
    int64_t dct_size[3];          /* requested block size per axis z,y,x (2D: [0] is ignored), each >= 1               */
    int64_t output_chunksize[3];  /* per-axis clamp of the block size, read when has_output_chunksize                 */
    double exponent;              /* exponent (weights.py:80)                                                          */
    double otf_support_fraction;  /* read when has_otf; has_otf == 0 is otf_support_fraction=None (the L1 branch)      */
    int32_t has_otf;
    int32_t has_output_chunksize;
} mvs_dct_opts_t;

/* mvs_fuse_chunk_dct == fuse_np(fusion_func=weighted_average_fusion, weights_func=content_based_dct) for one chunk
 * (fusion/_core.py:1620-1713, weights.py:77-290): every view is resampled onto the chunk (NaN outside), per view and
 * block of the chunk the DCT-entropy quality is computed (blocks anchored at chunk index 0, sizes per `dopts` clamped to
 * the chunk), the quality grids are shifted by their minimum over the views and normalised, and the weighted average of
 * mvs_fuse_chunk runs with every view's weight multiplied by its trilinear, clamped lookup into its grid.  opts->weights
 * must be MVS_WEIGHTS_NONE, opts->fusion MVS_FUSE_WEIGHTED_AVERAGE, opts->index_origin and the views' index_offset 0.
 * Option "dct_general" = 1: the quality pass takes its general path (global scratch) even for blocks of <= 32 per axis. */
int mvs_fuse_chunk_dct(int device, const mvs_view_t* views, int32_t n_views, const mvs_fuse_opts_t* opts,
                       const mvs_dct_opts_t* dopts, void* out);

/* mvs_content_dct_weights == weights.content_based_dct on a float32 stack `views` (n_views x shape, z,y,x; 2D data as
 * shape[0] == 1; NaN = outside the view): writes the normalised weights (n_views x shape, float32) to weights_out and,
 * when quality_out is not NULL, the raw per-block qualities (n_views x nb0 x nb1 x nb2, before the shift by the minimum)
 * to quality_out.  views, weights_out and quality_out all live in `mem` (MVS_MEM_HOST or MVS_MEM_DEVICE). */
int mvs_content_dct_weights(int device, const float* views, int32_t n_views, const int64_t shape[3], int32_t ndim,
                            const mvs_dct_opts_t* opts, float* weights_out, float* quality_out, int32_t mem);

/* ---- multi-view deconvolution ------------------------------------------------- *
 * Options of mvs_mv_deconv (fusion/mv_deconv.py:251-264 of the reference). */
typedef struct mvs_deconv_opts_t {
    int32_t n_iterations;  /* n_iterations (mv_deconv.py:255)                                  */
    int32_t erosion_px;    /* sample_boundary_erosion_px (:261, applied at :485-499)           */
    double lambda_reg;     /* Tikhonov strength; 0 = off (:256, :468-479)                      */
    double min_value;      /* clamp of the estimate and of the denominators (:257), used as float32 */
    int64_t trim[3];       /* halo trimmed off the result per axis z,y,x (fusion/_core.py:1687-1711) */
    int32_t out_dtype;     /* enum mvs_dtype of the result: nan_to_num + astype (_core.py:1713; :501) */
    int32_t flags;         /* MVS_DECONV_PREPARE_WEIGHTS: `weights` holds raw blending weights (mvs_blend_weights); they are
                              masked by the views' coverage and normalised in place first (_core.py:1648-1649,
                              weights.py:325-345) */
} mvs_deconv_opts_t;
#define MVS_DECONV_PREPARE_WEIGHTS 1

/* mvs_mv_deconv == fusion.multi_view_deconvolution (fusion/mv_deconv.py:251-501): Richardson-Lucy with sequential
 * per-view updates, every step on the device.  views / weights: device float32, n_views x shape (z,y,x; 2D data as
 * shape[0] == 1), NaN in a view = outside it, weights normalised (fusion/_core.py:1640-1649) unless opts->flags says otherwise.  kernels1 / kernels2: host
 * float32, n_views x ksize each, the forward PSFs and the compound back-projection kernels (:363-404) in
 * scipy.ndimage.convolve orientation (out[i] = sum_j k[j] in[i + K//2 - j]); every axis <= 63, else MVS_ERR_UNSUPPORTED.
 * sep1 / sep2 (both or neither; NULL = general path): host float32, n_views x (kz + ky + kx) 1-D factors (z, y, x) whose
 * outer product is the kernel of the same view -- the three-pass separable path.  Init (:409-414), forward convolution
 * with mode "mirror" + quotient + weighting (:434-462), back-projection with mode "constant", cval 1 + update (:464-483),
 * erosion of the union coverage (:485-499); then the result is trimmed by opts->trim, nan_to_num'd and cast to
 * opts->out_dtype into `out` (shape - 2 trim; host or device per out_mem).  A device result is not waited for. */
int mvs_mv_deconv(int device, const float* views, float* weights, int32_t n_views, const int64_t shape[3], int32_t ndim,
                  const float* kernels1, const float* kernels2, const int64_t ksize[3], const float* sep1, const float* sep2,
                  const mvs_deconv_opts_t* opts, void* out, int32_t out_mem);

/* ---- multi-band pyramid fusion -------------------------------------------------- *
 * Options of mvs_multiband_fuse. */
typedef struct mvs_multiband_opts_t {
    int32_t levels[3];        /* L_d >= 0: decimations of axis z,y,x (2D data: levels[0] == 0); at most 6               */
    int64_t index_origin[3];  /* global output-grid index of the array's first sample per axis: REDUCE keeps GLOBAL even
                                 indices, so every chunk of one stack decimates on the same lattice                      */
    int64_t trim[3];          /* halo trimmed off the result per axis z,y,x                                              */
    int32_t out_dtype;        /* enum mvs_dtype of the result; integers: round half to even, saturate (mvs_intensity_apply) */
    int32_t flags;            /* reserved, 0                                                                             */
} mvs_multiband_opts_t;

/* mvs_multiband_fuse: multi-band blending (Burt & Adelson 1983) of n_views resampled views.  views / weights: device float32,
 * n_views x shape (z,y,x; 2D data as shape[0] == 1); V: NaN (any non-finite) = outside the view; B: raw blending weights >= 0.
 * Pointwise:  m_v = isfinite(V_v);  w_v = m_v ? B_v : 0;  cov = sum w > 0;  W_v = cov ? w_v / sum w : 0;  I_v = m_v ? V_v : 0;
 *   F0 = sum_v W_v I_v;  D_v = m_v ? I_v - F0 : 0;  A_v = cov && v == argmax_u w_u (the lowest index wins ties; the float32 values
 *   themselves are compared).
 * Pyramid:  level l+1 decimates axis d only if levels[d] > l; L = max_d levels[d].  REDUCE along a decimated axis: taps
 *   [1,4,6,4,1]/16, samples kept at GLOBAL even indices, samples outside the array 0; level l+1 holds EVERY coarse sample whose 5-tap
 *   window meets level l's extent [s, s+n): K from ceil((s-2)/2) to floor((s+n+1)/2).  EXPAND along a decimated axis: global even
 *   g = 2K: (c[K-1] + 6 c[K] + c[K+1]) / 8; odd g = 2K+1: (c[K] + c[K+1]) / 2; missing coarse samples 0.  Both separable, axis order z,y,x.
 * Blend and collapse, l = L .. 0, with gD, gA the reduced D_v, A_v:  Ahat_{v,l} = gA_{v,l} / sum_u gA_{u,l} where that sum is > 0,
 *   else 0;  lap_{v,l} = gD_{v,l} - EXPAND(gD_{v,l+1}) (top level: gD_{v,L});  r_l = sum_v Ahat_{v,l} lap_{v,l} + EXPAND(r_{l+1}),
 *   summed in view order.
 * Result: cov ? F0 + r_0 : 0, trimmed by opts->trim and cast to opts->out_dtype into `out` (shape - 2 trim; host or device per
 *   out_mem).  Where the views agree or only one covers, the result is F0; levels 0 is the hard-seam mosaic; the result at a voxel
 *   depends on inputs within 4 (2^levels[d] - 1) voxels per axis.  Every sum has a fixed order: equal inputs give equal bits, and a
 *   voxel gets the same bits in any chunk that holds that radius around it.  A device result is not waited for.
 * MVS_ERR_UNSUPPORTED (never a crash): n_views < 1 or > 254, ndim not 2 or 3, a level < 0 or > 6. */
int mvs_multiband_fuse(int device, const float* views, const float* weights, int32_t n_views, const int64_t shape[3], int32_t ndim,
                       const mvs_multiband_opts_t* opts, void* out, int32_t out_mem);

/* ---- registration ------------------------------------------------------------ *
 * mvs_phasecorr == skimage.registration.phase_cross_correlation(fixed, moving,
 * normalization=None|"phase", upsample_factor=u, disambiguate=False)[0] as
 * called from registration.py:422-431:  F=fftn(a), G=fftn(b), P=F*conj(G),
 * [P /= max(|P|, 100 eps)], cc = ifftn(P), integer peak = argmax|cc| (lowest
 * flat index wins ties), wrap to signed shift, then upsampled-DFT refinement.
 * Inputs are float32, NaN-free, same shape; complex64 arithmetic.
 *   shift_out[3]      final (sub-pixel) shift, z,y,x (0 for the unused z in 2D)
 *   peak_index_out[3] integer argmax index before wrapping (bit-exact target)
 *   peak_abs_out      |cc| at that index                                        */
int mvs_phasecorr(int device, const float* fixed, const float* moving, int32_t mem,
                  int32_t ndim, const int64_t shape[3], int32_t normalization,
                  int32_t upsample_factor, double shift_out[3],
                  int64_t peak_index_out[3], float* peak_abs_out);
/* In-place complex64 (interleaved re, im) transform of one C-contiguous (z,y,x) array == numpy.fft.fftn /
 * ifftn (inverse != 0: conjugate transform WITHOUT the 1/N).  Any axis length up to 2^22 (powers of two: register /
 * LDS Stockham up to 4096, four-step in device scratch beyond; other lengths: Bluestein on the same cores, four-step above
 * 2048; longer axes return MVS_ERR_UNSUPPORTED).  The building block of mvs_phasecorr, exposed for tests and custom
 * pairwise registration functions. */
int mvs_fft_c2c(int device, void* data, int32_t mem, int32_t ndim, const int64_t shape[3], int32_t inverse);
/* The same for n_norm normalisations of ONE image pair (the reference calls phase_cross_correlation
 * with "phase" and None on the same inputs, registration.py:413-431): the two forward transforms
 * are computed once.  shifts_out: n_norm x 3, peak_indices_out: n_norm x 3 (may be NULL),
 * peak_abs_out: n_norm (may be NULL). */
int mvs_phasecorr_multi(int device, const float* fixed, const float* moving, int32_t mem,
                        int32_t ndim, const int64_t shape[3], const int32_t* normalizations,
                        int32_t n_norm, int32_t upsample_factor, double* shifts_out,
                        int64_t* peak_indices_out, float* peak_abs_out);
/* mvs_phasecorr_multi -- the same launches -- that also hands out what the upsampled-DFT refinement computed, for tests of
 * its kernels.  refined_out: n_norm blocks of U^ndim complex64 values (interleaved re, im), U = ceil(1.5 upsample_factor),
 * in the order [(uz,) uy, ux].  They are skimage's _upsampled_dft(image_product.conj(), ...) BEFORE its final .conj() (the
 * kernels form k * conj(v)); the sub-pixel maximum is the arg max of their moduli either way.  The values are in the units
 * of skimage's: the cross power the refinement reads is stored without the channel scales of the packed inverse transform.
 * refined_capacity counts floats: below 2 * n_norm * U^ndim, or refined_out NULL, returns MVS_ERR_INVALID_ARG before
 * anything runs.  upsample_factor == 1 has no refinement: nothing is written and refined_out may be NULL. */
int mvs_phasecorr_multi_refined(int device, const float* fixed, const float* moving, int32_t mem,
                                int32_t ndim, const int64_t shape[3], const int32_t* normalizations,
                                int32_t n_norm, int32_t upsample_factor, double* shifts_out,
                                int64_t* peak_indices_out, float* peak_abs_out, float* refined_out,
                                int64_t refined_capacity);

/* Intensity normalisation of one registration input == skimage.exposure.rescale_intensity(im,
 * in_range=(nanmin(im), nanmax(im)), out_range=(0, 1)) as called at registration.py:381-389:
 * float32 in/out, NaN preserved; also reports nanmin, nanmax and the number of non-NaN voxels
 * (valid_pixels1 of registration.py:400). */
int mvs_rescale_intensity(int device, const float* in, int32_t mem, int64_t n, float* out, int32_t out_mem,
                          float* min_out, float* max_out, int64_t* nvalid_out);

/* Block-mean binning of one view == sim.coarsen(bins, boundary="trim").mean().astype(dtype)
 * (registration.py:1732-1741): out shape = shape // bin; the mean is sum / count in double (a true division, as numpy's: a
 * block whose sum is a multiple of its count gives exactly that integer for every count), cast like astype. */
int mvs_bin_mean(int device, const void* in, int32_t dtype, int32_t mem, const int64_t shape[3],
                 const int64_t stride[3], const int64_t bin[3], void* out, int32_t out_mem);

/* mvs_bin_mean between device buffers without the final wait: the kernel is queued on the context lane's stream and the
 * call returns; mvs_synchronize(device) orders later use (other lanes read the result only after it).  Lets a host that
 * has other work -- registration.register builds and prunes its overlap graph -- bin all tiles of a mosaic meanwhile
 * (reference: the same coarsen().mean() of registration.py:1732-1741, there part of the lazy dask graph). */
int mvs_bin_mean_async(int device, const void* in, int32_t dtype, const int64_t shape[3], const int64_t stride[3],
                       const int64_t bin[3], void* out);

/* mvs_bin_mean_async for n_views views of one shape, stride and dtype (in[v] -> out[v], device memory) in one call: the
 * binning of all tiles of a mosaic is queued with one library call (16-bit tiles binned by 2 along x: one launch per 32 views). */
int mvs_bin_mean_batch_async(int device, int32_t n_views, const void* const* in, int32_t dtype, const int64_t shape[3],
                             const int64_t stride[3], const int64_t bin[3], void* const* out);

/* Stream-ordered dependencies between context lanes, no host wait (the reference's dask graph orders the binning of a view
 * before the pairs that read it, registration.py:1732-1741 -> 2657-2664; here the binning runs on one lane and the pairs on
 * the others).  mvs_event_record marks the work queued so far on this lane and returns a ticket; mvs_event_wait(device,
 * ticket) makes the work queued LATER on `device`'s lane wait for that mark.  A lane keeps 32 tickets: an older one stands for
 * the mark that replaced it (the wait is longer, never shorter). */
int mvs_event_record(int device, uint64_t* ticket_out);
int mvs_event_wait(int device, uint64_t ticket);

/* ---- Transfers that overlap with the kernels (csrc/mvs_transfer.hip).  The reference's users hand fuse() host- or Zarr-backed
 * arrays and stream the fused chunks out (fusion/_core.py:1068-1170, 2044-2156; spatial_image_utils.py:712-860); SURVEY 8d(2)
 * counts H2D / D2H into the end-to-end figure.  mvs_host_alloc: pinned host memory (what an asynchronous copy needs to be
 * asynchronous).  mvs_copy_async: one copy (kind 0: host -> device, 1: device -> host) on the device's COPY STREAM of that direction -- one
 * per device and direction (uploads and downloads run side by side, each direction in the order queued), created with a priority of
 * their own so that queued copies do not stall the compute streams -- started after ticket
 * `after` (0: at once; a ticket of mvs_event_record, mvs_mark or an earlier mvs_copy_async) and marked by the ticket *done_out.
 * Tickets of this group are timed events from a ring of 4096 per device; mvs_event_wait accepts them, so a pair job of
 * mvs_register_pairs (wait_ticket) starts when its two tiles have landed, and a download starts when the launch that produced
 * its data is done (mvs_mark on the producing lane).  mvs_ticket_sync: the host waits for a ticket; mvs_ticket_elapsed_ms: the
 * time between two tickets of one device (both must have passed or the call waits for them).  Host pointers must stay valid, and
 * unchanged for uploads, until the ticket has passed. */
int mvs_host_alloc(uint64_t nbytes, void** host_ptr);
int mvs_host_free(void* host_ptr);
int mvs_copy_async(int device, void* dst, const void* src, uint64_t nbytes, int32_t kind, uint64_t after, uint64_t* done_out);
int mvs_mark(int device, uint64_t* ticket_out);
int mvs_ticket_sync(uint64_t ticket);
int mvs_ticket_elapsed_ms(uint64_t t0, uint64_t t1, double* ms_out);

/* Candidate scoring == the loop of registration.py:493-556 for n translation
 * candidates t (z,y,x rows): moving resampled by t (order 1, NaN outside),
 * masks, bounding-box region (region_mode 0 = "union", 1 = "intersection"),
 * SSIM (ssim_out) and masked Spearman correlation (spearman_out).  A skipped
 * candidate reports code_out = 1 (mask empty / <10% valid -> both metrics -1),
 * 2 (the `continue` of registration.py:530-533, no metric appended), else 0.
 * quality_for_all = 0: the rank correlation is evaluated only for the candidate(s)
 * holding the best SSIM -- the only one the reference reports (registration.py:543-556) --
 * and spearman_out is NaN for the other scored candidates; 1: for every candidate. */
int mvs_score_candidates(int device, const float* fixed, const float* moving, int32_t mem,
                         int32_t ndim, const int64_t shape[3],
                         const double* t_candidates, int32_t n_candidates,
                         int32_t region_mode, double data_range, double im1_min,
                         int32_t quality_for_all,
                         double* ssim_out, double* spearman_out, int32_t* code_out);
/* mvs_score_candidates as mvs_register_crops calls it -- only the arg max is needed, so the pruned arg-max search (option
 * "ssim_prune") and its float32 walk (option "ssim_f32") may run: the same launches -- that also hands out what the search knew
 * about every candidate, for tests of the walk kernels and of the hand-over between them.  value_bound: the largest absolute value
 * of the two (rescaled) crops (the search runs when 1e-2 max(1, (value_bound / data_range)^2) <= 0.05).  The rank correlation
 * is evaluated for the best-SSIM candidate(s) only (quality_for_all = 0).  Per candidate with code_out 0:
 * state_out: MVS_SCORE_COMPLETE = walked over its whole volume; MVS_SCORE_DROPPED = left unfinished, ssim_out then holds the
 * bound its mean could not exceed (below the best mean); MVS_SCORE_REWALKED = walked again by the float64 kernel, ssim_out is that
 * walk's mean.  ssim_rounds_out: the mean SSIM the candidate had when the rounds ended, before any re-walk (NaN unless complete).
 * A call that does not take the pruned search reports MVS_SCORE_COMPLETE and ssim_rounds_out = ssim_out.  Candidates with another
 * code report state 0 and NaN.  Both arrays are required (NULL: MVS_ERR_INVALID_ARG).  Option "ssim_f32" = 0 (default 1): the
 * rounds of the search run in float64 and nothing is walked again; counter "reg_rewalks": candidates walked again in float64
 * (each also counts one volume in "reg_cand_volumes"). */
#define MVS_SCORE_COMPLETE 1
#define MVS_SCORE_DROPPED 2
#define MVS_SCORE_REWALKED 4
int mvs_score_candidates_argmax(int device, const float* fixed, const float* moving, int32_t mem,
                                int32_t ndim, const int64_t shape[3],
                                const double* t_candidates, int32_t n_candidates,
                                int32_t region_mode, double data_range, double im1_min, double value_bound,
                                double* ssim_out, double* spearman_out, int32_t* code_out,
                                double* ssim_rounds_out, int32_t* state_out);

/* The whole of registration.phase_correlation_registration (registration.py:353-565) for two same-shape
 * float32 overlap crops (NaN = outside the view) in one call: intensity normalisation, the two phase
 * correlations, the zero-shift candidate when a crop holds NaNs (quirk Q1), candidate enumeration, scoring and
 * the nanargmax selection with the reference's list bookkeeping (quirk Q3).  upsample_factor: the reference uses
 * 10 in 2D and 2 in 3D; region_mode -1 = the reference's choice ("intersection" with NaNs, else "union");
 * constant_check != 0 adds dispatch_pairwise_reg_func's guard (registration.py:1500-1520).
 * t_out: translation (z,y,x; fixed px -> moving px), quality_out: Spearman coefficient of the selected candidate.
 * status_out: 0 = ok, 1 = no admissible candidate (the reference returns [zeros(ndim)], quirk Q2),
 * 2 = constant crop (identity, quality NaN), 3 = no finite SSIM (np.nanargmax raises in the reference). */
int mvs_register_crops(int device, const float* fixed, const float* moving, int32_t mem, int32_t ndim,
                       const int64_t shape[3], int32_t upsample_factor, int32_t region_mode,
                       int32_t constant_check, double t_out[3], double* quality_out,
                       int32_t* status_out, int32_t* n_candidates_out);

/* One call per image pair == sims_to_intrinsic_coord_system + dispatch_pairwise_reg_func(phase_correlation_registration)
 * (registration.py:280-350, 1477-1544, 353-565): both views (mvs_view_t geometry as for mvs_resample: matrix / offset map
 * pixels of the fixed view's overlap grid to pixels of the view's slab) are resampled with order 1 and NaN outside onto
 * out_shape (float32, library scratch) and handed to mvs_register_crops without a host round trip in between.  Outputs as
 * mvs_register_crops. */
int mvs_register_views(int device, const mvs_view_t* fixed_view, const mvs_view_t* moving_view, int32_t ndim,
                       const int64_t out_shape[3], int32_t upsample_factor, int32_t region_mode, int32_t constant_check,
                       double t_out[3], double* quality_out, int32_t* status_out, int32_t* n_candidates_out);

/* All pairs of a mosaic in one call (registration.compute_pairwise_registrations, registration.py:2622-2714: one task per
 * pair; here one library call, the pairs farmed over context lanes by native worker threads -- no interpreter in the loop).
 *
 * mvs_plan_pairs (host only): for pairs of views whose transform is a pure translation, what register_pair_of_msims ->
 * sims_to_intrinsic_coord_system -> get_pixel_affine derive per pair (registration.py:194-350, 1547-2058; transformation.py:37-83).
 * coords[v * ndim + k]: the coordinate array of view v along axis k (coord_len entries; origin = c[0], spacing = c[1] - c[0]);
 * translation: n_views x ndim; tol: ndim overlap tolerances or NULL; pairs: n_pairs x 2 (fixed, moving).  Per pair p:
 * windows_out[((p * 2 + i) * 3 + k) * 2 + {0, 1}] = first / one-past-last index of view i's crop window on axis k (the overlap
 * + one sample + 1e-6 on either side), out_origin / out_spacing / out_shape (p * 3 + k) = the fixed view's overlap grid,
 * matrix_diag / offset ((p * 2 + i) * 3 + k) = the pixel affine of crop i (output pixel -> window pixel; rounded to 10
 * decimals, offsets within 1e-6 of an integer snapped), status_out[p] = 0 ok, 1 the views do not overlap.  Axes k < ndim.
 *
 * mvs_register_pairs: mvs_register_views for every job on n_lanes (<= 16) native worker threads, thread w driving context lane
 * `device | w << 8`; `device` carries no lane.  wait_ticket: mvs_event_record tickets (0 = none) the lane's stream waits for
 * before it reads the fixed / moving view (binned tiles still being produced on another lane).  Outputs per pair as
 * mvs_register_views (t_out: n_pairs x 3); rc_out[p] = that pair's return code.  Returns 0, or the first failing pair's code
 * with its message in mvs_last_error(device). */
typedef struct mvs_pair_job_t {
    mvs_view_t fixed;
    mvs_view_t moving;
    int64_t out_shape[3];
    uint64_t wait_ticket[2];
    int32_t bin[3];          /* bin[0] > 0: `fixed` / `moving` are windows of RAW uint8 / uint16 tiles (shape = a whole number of bins
                                per axis, identity matrix, offset = the whole-pixel translation in BINNED pixels) and the crops are
                                taken with this registration binning applied on the fly -- sim.coarsen(bin).mean().astype(dtype)
                                (registration.py:1732-1741) and the crop in one pass, no binned copy of the tiles; all zero: the
                                views are used as they are (mvs_register_views) */
    int32_t flags;           /* bit 0: when the pair is done, wait_ticket[0] is OVERWRITTEN with a timed ticket (mvs_mark) of the pair's
                                lane -- when its last kernel finished, for timelines (mvs_ticket_elapsed_ms); 0: the job is only read */
} mvs_pair_job_t;
int mvs_plan_pairs(int32_t ndim, int32_t n_views, const double* const* coords, const int64_t* coord_len, const double* translation,
                   const double* tol, int32_t n_pairs, const int32_t* pairs, int64_t* windows_out, double* out_origin_out,
                   double* out_spacing_out, int64_t* out_shape_out, double* matrix_diag_out, double* offset_out, int32_t* status_out);
int mvs_register_pairs(int device, int32_t n_pairs, mvs_pair_job_t* jobs, int32_t ndim, int32_t upsample_factor,
                       int32_t region_mode, int32_t constant_check, int32_t n_lanes, double* t_out, double* quality_out,
                       int32_t* status_out, int32_t* n_candidates_out, int32_t* rc_out);

/* Host-only (no device, no mvs_init needed): the inner loop of the reference's global optimisation for the translation
 * model -- optimize_bead_subgraph, param_resolution/global_optimization.py:313-417 with transforms.py:45-53 as estimator.
 * Edge e joins nodes edge_nodes[2e], edge_nodes[2e+1] and carries n_beads virtual beads in each node's frame
 * (beads_a / beads_b: n_edges x n_beads x ndim doubles, param_resolution/utils.py:42-78).  Sweep: the nodes in `order`
 * (ref_node and nodes without edges are skipped) each add mean(adjacent bead - own bead), taken in world coordinates over
 * all their beads, to their translation.  After each sweep the bead residuals |a + t_a - b - t_b| are stored
 * (edge_residuals: n_edges x n_beads), their mean of edge means and maximum are appended to mean_hist / max_hist
 * (max_iter doubles each); from the 7th sweep on the loop stops when max |r - r_previous| / max r < rel_tol.
 * translations (n_nodes x ndim) is in/out; n_iter_out = sweeps done.
 * Contract with the numpy form of the same sweeps (param_resolution.py, used for the models with a linear part): the node
 * update is evaluated in affine form (sum over a node's edges of +-(D0_e + n_beads (T_a - T_b))), i.e. its additions run in
 * another order than the bead-by-bead sum -- equal to 1e-10 in translations, residuals and both histories, NOT bit for bit
 * (tests/test_param_resolution.py).  The AVX2 residual pass (x86-64 hosts that have it) equals the scalar loops bit for bit. */
int mvs_beads_translation_sweeps(int32_t ndim, int32_t n_nodes, int32_t n_edges, const int32_t* edge_nodes,
                                 const double* beads_a, const double* beads_b, int32_t n_beads, const int32_t* order,
                                 int32_t ref_node, int32_t max_iter, double rel_tol, double* translations,
                                 double* edge_residuals, double* mean_hist, double* max_hist, int32_t* n_iter_out);

/* Host-only: the chunk -> view-slab plan of fusion.fuse (fusion/_core.py:354-722 with mv_graph.py:934-1117 and the label
 * selection of _core.py:1371-1386).  All per-axis arrays hold `ndim` entries per item in (z,) y, x order: views as
 * origin / spacing / shape of their stacks and (ndim + 1)^2 row-major affines `params` (view -> world; `inv_params` = their
 * inverses, needed -- and only read -- when some view is not a pure translation), the output stack, the chunk size and the
 * halo (overlap_in_pixels).  Decides which axes are pure translations for every view (dim_masks_out[0], bit d = axis d) and on
 * which of those the output samples fall on every view's sampling grid (dim_masks_out[1]: no interpolation taps there,
 * _core.py:354-459), then lists, in block order (first axis slowest) and ascending view index, one entry per (output chunk,
 * contributing view): the integer window lo[d] .. lo[d] + n[d] - 1 of the view that the chunk (grown by the halo and by
 * `interpolation_order` taps on the axes that interpolate) needs (_core.py:462-533 for translations, mv_graph.py:989-1117
 * for general affines), exactly the samples the reference's `sims[iview].sel(...)` selects.  planewise = 1 when the chunk is a
 * single z plane on the views' z grid (fused with the 2D parameters, _core.py:694-703).  Call with entries = NULL to get
 * the count in n_entries_out, then with capacity >= that count. */
typedef struct mvs_plan_entry {
    int64_t block[3];
    int32_t view;
    int32_t planewise;
    int64_t lo[3];
    int64_t n[3];
} mvs_plan_entry_t;
int mvs_fuse_plan(int32_t ndim, int32_t n_views, const double* view_origin, const double* view_spacing, const int64_t* view_shape,
                  const double* params, const double* inv_params, const double* out_origin, const double* out_spacing,
                  const int64_t* out_shape, const int64_t* chunk_size, const int64_t* halo, int32_t interpolation_order,
                  mvs_plan_entry_t* entries, int64_t capacity, int64_t* n_entries_out, int32_t* dim_masks_out);

/* Host-only: edge betweenness centrality of the view adjacency graph -- networkx.edge_betweenness_centrality(g) as
 * prune_graph_to_alternating_colors calls it (mv_graph.py:664-741; Brandes, unweighted, normalised by n (n - 1)).  Nodes are
 * 0 .. n_nodes - 1 in the graph's node order, node v's neighbours adj_nodes[adj_offsets[v] .. adj_offsets[v + 1]) in
 * adjacency order, adj_edge[a] = index of the edge adjacency entry a belongs to; bet_out: n_edges doubles.  Traversal and
 * accumulation order are networkx's (the reference compares the derived edge values with <=). */
int mvs_edge_betweenness(int32_t n_nodes, int32_t n_edges, const int32_t* adj_offsets, const int32_t* adj_nodes,
                         const int32_t* adj_edge, double* bet_out);

/* Host-only: the pairs registration.register registers, for views whose world frames are axis-aligned boxes -- the overlap
 * graph of mv_graph.build_view_adjacency_graph_from_msims (mv_graph.py:35-180) and, with method 1, its pruning by
 * prune_graph_to_alternating_colors (mv_graph.py:664-741, the default pre_registration_pruning_method) in one call.
 * box_lo / box_hi: n_views x ndim world coordinates of the first / last sample of every view (after any overlap tolerance);
 * pairs: n_pairs x 2 candidate view indices in the order the reference's cKDTree ball query lists them (i != j; (j, i) after
 * (i, j) changes nothing).  An unordered pair becomes an edge at its first appearance when its intersection volume
 * prod(min(hi) - max(lo)) is positive on every axis (the value Qhull returns for the box).  method 0: all edges; method 1:
 * edges are removed level by level in rising order of overlap + betweenness bonus (an edge with an end point of degree 1 stays)
 * until a greedy largest-first colouring needs at most n_colors colours.  Output: the surviving edges in networkx's edges()
 * order (node by node, neighbours in insertion order), each (i, j) with i < j, and their overlap volumes; edges_out holds
 * 2 * n_pairs int32, overlap_out n_pairs doubles at most.  n_graph_edges_out (optional): edges before pruning.
 * MVS_ERR_UNSUPPORTED: a case the Python form decides (NaN volumes, no colouring within the levels). */
int mvs_view_graph_prune(int32_t ndim, int32_t n_views, const double* box_lo, const double* box_hi, int64_t n_pairs,
                         const int32_t* pairs, int32_t method, int32_t n_colors, int32_t* edges_out, double* overlap_out,
                         int32_t* n_edges_out, int32_t* n_graph_edges_out);

/* Host-only: param_resolution.groupwise_resolution(method="global_optimization", transform="translation")
 * (param_resolution/__init__.py:44-150, global_optimization.py:16-511, utils.py:42-101) for a CONNECTED mosaic whose pairwise
 * results are pure translations, in one call.  edges: n_edges x 2 view indices (i < j) in the order the pairs were added to the
 * registration graph; pair_t: n_edges x ndim translation of each pair's transform; quality: n_edges; bbox_lo / bbox_hi:
 * n_edges x ndim overlap box of each pair in the fixed view's frame; spacing: n_views x ndim (abs_tol < 0: the largest voxel
 * diagonal is used).  reference_view < 0: the view with the largest sum of edge qualities.  Outputs: translations_out
 * (n_views x ndim, the reference view keeps 0), edge_rms_out (n_edges, RMS bead residual per edge in input edge order),
 * mean_hist / max_hist (max_iter doubles each: mean of edge means / maximum of the bead residuals after every sweep),
 * n_iter_out, ref_out (optional).  Returns MVS_ERR_UNSUPPORTED -- and the caller takes the Python form -- when the graph is not
 * one component over all views, an edge is duplicated, an input is not finite, or the final maximal residual is not below
 * abs_tol (the reference then starts removing edges: global_optimization.py:419-505). */
int mvs_resolve_translations(int32_t ndim, int32_t n_views, int32_t n_edges, const int32_t* edges, const double* pair_t,
                             const double* quality, const double* bbox_lo, const double* bbox_hi, const double* spacing,
                             int32_t reference_view, int32_t max_iter, double rel_tol, double abs_tol, double* translations_out,
                             double* edge_rms_out, double* mean_hist, double* max_hist, int32_t* n_iter_out, int32_t* ref_out);

/* Normal equations of one Gauss-Newton step of the intensity registration (registration.affine_registration) over two
 * same-shape C-contiguous float32 crops (NaN = outside), both in `mem`.  matrix (3x3 row-major, z,y,x) and offset hold the
 * centred pose: fixed voxel x samples moving at p = c + t + A (x - c), c = (shape - 1) / 2.  ndim 2: shape = (1, ny, nx) and
 * only the lower right 2x2 of matrix and the last two entries of offset are read.  Per voxel (arithmetic and operation order:
 * csrc/mvs_affine_reg_dev.h): p in double, split into floor and a float32 fraction; the sample counts iff F(x) is finite, all
 * 2^ndim taps lie inside moving and all are finite; then in float32 the bi/trilinear value v, the analytic gradient g of the
 * interpolant, r = gain v + bias - F and J = gain g (x) [x - c, 1] (parameters: the rows of [A | t], P = ndim (ndim + 1)).
 * out (MVS_AFFINE_NEQ_LEN doubles, packed for the given ndim, the rest zero): J^T J as a full P x P matrix, J^T r (P),
 * sum r^2, the valid count, then sum v, sum F, sum v F, sum v^2, sum F^2.  Threads sum runs of 32 samples in float32,
 * everything above in double, in a fixed order: equal inputs give equal bits.  Runs on the context lane of `device`. */
#define MVS_AFFINE_NEQ_LEN (12 * 12 + 12 + 7)
int mvs_affine_normal_eq(int device, const float* fixed, const float* moving, int32_t mem,
                         int32_t ndim, const int64_t shape[3],
                         const double matrix[9], const double offset[3],
                         double gain, double bias, double* out);

/* Mattes mutual information of the same warped crop pair (registration.affine_registration, metric="mattes").  Crops, mem,
 * ndim, shape, matrix, offset, the warp and the rule for a valid sample: as mvs_affine_normal_eq.  n_bins = B in 8..64.  Per valid
 * sample, in float32 (arithmetic and operation order: csrc/mvs_affine_mi_dev.h): the fixed bin a = clamp(floor((F - f_lo) *
 * f_scale + 0.5), 0, B - 1); the moving coordinate u = clamp((v - m_lo) * m_scale + 1.5, 1.5, B - 2.5) with its four taps
 * b_k = floor(u) - 1 + k; the cubic B-spline window beta3(u - b_k).  The caller passes f_scale = (B - 1) / (f_hi - f_lo) and
 * m_scale = (B - 4) / (m_hi - m_lo) for the finite ranges of the two crops (mvs_finite_range).
 *
 * mvs_affine_joint_hist: hist_out[a * B + b_k] += (int64)(beta3(u - b_k) * 2^20 + 0.5) over all valid samples (B * B values, host
 * memory), *n_valid_out = their number.  The weights are integers, so the sums do not depend on their order: the kernel adds with
 * integer atomics (LDS, then global) and equal inputs still give equal bits.
 *
 * mvs_affine_mi_gradient: table (B * B float32, host memory: L[a][b]); per valid sample w = sum_k beta3'(u - b_k) * L[a][b_k] in
 * float32 in k order.  out (MVS_AFFINE_MI_GRAD_LEN doubles, packed for the given ndim, the rest zero): sum w g_j (x - c)_i and
 * sum w g_j in the order of the rows of [A | t] (P = ndim (ndim + 1) values, the monomials of J^T r of mvs_affine_normal_eq), then
 * the valid count.  Threads sum runs of 32 samples in float32, everything above in double, in a fixed order, no floating-point
 * atomics: equal inputs give equal bits.  Both wait for their result and run on the context lane of `device`. */
#define MVS_AFFINE_MI_GRAD_LEN (12 + 1)
int mvs_affine_joint_hist(int device, const float* fixed, const float* moving, int32_t mem,
                          int32_t ndim, const int64_t shape[3],
                          const double matrix[9], const double offset[3],
                          int32_t n_bins, float f_lo, float f_scale, float m_lo, float m_scale,
                          int64_t* hist_out, int64_t* n_valid_out);
int mvs_affine_mi_gradient(int device, const float* fixed, const float* moving, int32_t mem,
                           int32_t ndim, const int64_t shape[3],
                           const double matrix[9], const double offset[3],
                           int32_t n_bins, float f_lo, float f_scale, float m_lo, float m_scale,
                           const float* table, double* out);

/* Minimum, maximum and number of the finite values (neither NaN nor +-inf) of n float32 values in `mem`; NaN, NaN, 0 when there
 * is none.  Per-block partials, finished on the host.  Waits for the result; runs on the context lane of `device`. */
int mvs_finite_range(int device, const float* data, int32_t mem, int64_t n, float* min_out, float* max_out, int64_t* n_finite_out);

/* Bead detection (detection.log_detect), first half: the Laplacian-of-Gaussian response of a C-contiguous 2-D / 3-D image (uint8,
 * uint16 or float32, in `mem`; ndim 2: shape = (1, ny, nx)).  response (device memory, float32, the image's shape) becomes
 *   -scipy.ndimage.gaussian_laplace(image as float32, sigma, mode="reflect") * scale.
 * The host supplies the filter taps (scipy's _gaussian_kernel1d): radius[k] per axis (z, y, x; the z entry is ignored in 2D), and
 * taps0 / taps2 = the order-0 / order-2 tables of the image's axes one after the other, 2 radius + 1 float64 values each.  ndim
 * line passes carry two volumes (x: G I and G'' I; y: G A and G'' A + G B; z: the sum): float64 accumulation over the float64
 * taps in scipy's order, float32 stores after each pass.  The line ends reflect as scipy's do, also when the radius exceeds the
 * axis length and on an axis of one sample.  A radius above MVS_LOG_MAX_RADIUS returns MVS_ERR_UNSUPPORTED.
 * taps2 == NULL: response becomes scipy.ndimage.gaussian_filter(image as float32, sigma) instead (scale is not used).
 * *max_out (optional) = the maximum of response (NaN ignored) over the slices [max_range[0], max_range[1]) of the image's first
 * axis (max_range == NULL: all of it); per-workgroup maxima and a second small launch, no atomics.  Work area: ndim float32
 * volumes (one for smoothing) plus the image when it comes from the host.  Waits for the result; runs on the lane of `device`.
 * Both detection entry points return MVS_ERR_UNSUPPORTED for an axis above 2^24 or a volume above MVS_DETECT_MAX_VOXELS, and this
 * one also when a pass would need 2^24 workgroups or more (a tile is 64 x columns by 16 rows or 32 positions, so volumes with very
 * short rows reach that first). */
#define MVS_LOG_MAX_RADIUS 40
#define MVS_DETECT_MAX_VOXELS ((int64_t)1 << 34)
int mvs_log_response(int device, const void* image, int32_t dtype, int32_t mem, int32_t ndim, const int64_t shape[3],
                     const int32_t radius[3], const double* taps0, const double* taps2, double scale,
                     const int64_t* max_range, float* response, float* max_out);

/* Bead detection, second half: the voxels of a float32 device volume where
 *   r == maximum of r over the box window[] (odd sizes; z, y, x; mode "reflect"),  r > threshold  and  r > 0
 * hold (a NaN fails every comparison).  With sample != NULL (a device volume of sample_dtype and the same shape) a voxel also
 * needs  min of sample over its box sample_window[] < bound;  a window of size n at position i covers [i - n/2, i - n/2 + n - 1]
 * (even sizes allowed, as in scipy.ndimage.minimum_filter), and the minimum is evaluated at the remaining candidates only.  A
 * float32 sample is compared with (float)bound, an integer one exactly.  *count_out = the exact number of detections;
 * coords_out (host memory, capacity x 3 int32: z, y, x) receives min(count, capacity) of them in NO defined order (one integer
 * atomicAdd per wave appends them): sort for a deterministic list.  Window sizes go up to MVS_MAXIMA_MAX_WINDOW: every
 * output of a running maximum reads its whole window again, so a pass costs `window` loads per voxel (7 for a bead of 6 voxels;
 * the largest window log_detect derives under MVS_LOG_MAX_RADIUS is 37), and the box minimum costs the product of its sizes per
 * candidate.  Work area: ndim - 1 float32 volumes and the list.  Waits for the result; runs on the lane of `device`. */
#define MVS_MAXIMA_MAX_WINDOW 127
int mvs_local_maxima(int device, const float* response, int32_t ndim, const int64_t shape[3], const int32_t window[3],
                     float threshold, const void* sample, int32_t sample_dtype, const int32_t sample_window[3], double bound,
                     int32_t* coords_out, int64_t capacity, int64_t* count_out);

/* Registration quality metrics (metrics.tile_pair_image_metrics): the sample moments of a fixed and a moving tile over the
 * overlap grid of one directed pair, for up to MVS_PAIR_MAX_CANDIDATES candidate transforms of the moving tile in one pass.
 *   fixed->matrix / offset        grid index -> fixed pixel
 *   cand_matrix[k] / cand_offset[k]   grid index -> moving pixel under candidate k (9 + 3 doubles, the layout of mvs_view_t;
 *                                 the matrix / offset of `moving` itself are not read)
 *   halfspaces                    n_halfspaces rows (a_z, a_y, a_x, b) in GRID INDEX coordinates (0 .. MVS_PAIR_MAX_HALFSPACES rows)
 * The views are uint8, uint16 or float32 and share one dtype (else MVS_ERR_UNSUPPORTED), in host or device memory, possibly
 * strided windows (stride[2] == 1); host slabs are C-contiguous and staged as by mvs_resample.  ndim 2: grid_shape[0] == 1 and
 * shape[0] == 1 of both views.
 * Per grid voxel (z, y, x), all coordinate arithmetic in double without contraction:
 *   1. mask:   ((a_z z + a_y y) + a_x x) + b <= 0 for every halfspace (none given: every voxel passes);
 *   2. fixed sample: c = ((z m0 + y m1) + x m2) + offset per axis; in bounds iff 0 <= c <= n - 1 on every axis; the bi / trilinear
 *      sample of mvs_resample (order 1: float32 weights and taps, all taps read, so a NaN tap -- also one of weight 0 -- makes the
 *      sample NaN); computed once and used for every candidate;
 *   3. moving sample: the same under candidate k;
 *   4. the pair (f, m_k) counts for candidate k iff the mask holds, both samples are in bounds and both are finite.
 * out (host memory) receives n_candidates rows of MVS_PAIR_MOMENTS_LEN doubles
 *   n, mean_f, mean_m, M2_f = sum (f - mean_f)^2, M2_m = sum (m - mean_m)^2, C_fm = sum (f - mean_f)(m - mean_m)
 * over the counted pairs (n == 0: all six are 0).  Row k belongs to candidate k: callers keep the reference's order, the list
 * candidate_keys of metrics.py:550-555 (the query transform keys as given, or the single key "transform").  A candidate's row does
 * not depend on which other candidates share the launch.
 * Reduction: every thread takes one voxel per step of a grid-stride loop and keeps, per candidate, an integer count and float64
 * sums of the samples SHIFTED by its first counted pair (no raw sum of squares: a 16-bit tile at 60000 +- 3 keeps its variance,
 * a constant tile sampled without interpolation rounding has M2 == 0 exactly), turns them into a record (n, means, M2s, C) and
 * records are merged pairwise with the update of Chan, Golub and LeVeque in a fixed tree: the lanes of a wave by shuffles, the
 * waves of a workgroup through LDS, one record per workgroup in scratch, and a second launch (one wave per candidate: each lane
 * folds a run of consecutive records in index order, then the lanes merge).  No floating-point atomics and no completion
 * counters; the launch has min(ceil(voxels / MVS_PAIR_BLOCK_VOXELS), MVS_PAIR_MAX_BLOCKS) workgroups, a function of the voxel
 * count only, so equal inputs give equal bits.  Waits for the result; runs on the lane of `device`. */
#define MVS_PAIR_MOMENTS_LEN 6
#define MVS_PAIR_MAX_CANDIDATES 8
#define MVS_PAIR_MAX_HALFSPACES 16
#define MVS_PAIR_BLOCK_VOXELS 256
#define MVS_PAIR_MAX_BLOCKS 2048
int mvs_pair_moments(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int32_t n_candidates,
                     const double* cand_matrix, const double* cand_offset, int32_t ndim, const int64_t grid_shape[3],
                     const double* halfspaces, int32_t n_halfspaces, double* out);

/* Marker-based (bead) registration, registration.registration_marker_based (registration.py:595-1379): the three device entry
 * points below; thresholds, the ratio test, sampling, the model fits, ranking and the ICP bookkeeping are host work.  All
 * arithmetic on coordinates and distances is float64 without contraction; a distance is sqrt(sum_d (a_d - b_d)^2), summed over the
 * DIFFERENCES in axis order (world coordinates at 1e6 with sub-pixel differences keep their digits).  All three wait for their
 * result and run on the context lane of `device`.
 *
 * mvs_knn: brute-force k nearest neighbours, in the seat of the reference's cKDTree(...).query calls (registration.py:619, 662-664,
 * 743-746, 1095-1097).  ref: n_ref rows of dim float64, query: n_query rows, each C-contiguous in host or device memory (ref_mem /
 * query_mem); the same pointer for both (a set against itself) is staged once.  idx_out / dist_out (host memory, n_query x k):
 * the k nearest reference rows of every query, ascending by distance, equal distances by ascending reference index; with
 * k > n_ref the tail is index -1 and distance +inf.  A NaN distance never enters the list.  1 <= dim <= MVS_KNN_MAX_DIM (the
 * descriptor length C(num_neighbors + 1, 2) at num_neighbors = 5) and 1 <= k <= MVS_KNN_MAX_K, else MVS_ERR_UNSUPPORTED; at most
 * 2^30 rows per set.  One query per thread with its coordinates and its sorted top-k in registers (dim 1, 2, 3, 6, 10 and k 1, 2,
 * 8, 16 are compiled forms, other values take the next larger); reference rows pass through LDS in tiles of 256, component-major. */
#define MVS_KNN_MAX_DIM 15
#define MVS_KNN_MAX_K 16
int mvs_knn(int device, const double* ref, int32_t ref_mem, int64_t n_ref, const double* query, int32_t query_mem, int64_t n_query,
            int32_t dim, int32_t k, int32_t* idx_out, double* dist_out);

/* The geometric descriptors of registration.py:666-690.  points: n_points x ndim float64 (ndim 2 or 3) in points_mem; neighbors
 * (host memory): n_points x required int32, required = num_neighbors + redundancy -- each point's nearest OTHER points.  For point
 * p and subset s of its neighbours -- the C = C(required, num_neighbors) subsets in itertools.combinations order -- row p * C + s
 * of out (out_mem; n_points * C rows of num_neighbors (num_neighbors + 1) / 2 float64) is the ascending vector of all pairwise
 * distances among the point and the subset.  One thread per row; a fixed compare-exchange sequence sorts.  A neighbour index
 * outside [0, n_points) makes its rows NaN.  num_neighbors above MVS_MARKER_MAX_NEIGHBORS or required above MVS_KNN_MAX_K - 2
 * (the neighbourhood query takes required + 2): MVS_ERR_UNSUPPORTED. */
#define MVS_MARKER_MAX_NEIGHBORS 5
int mvs_marker_descriptors(int device, const double* points, int32_t points_mem, int64_t n_points, int32_t ndim,
                           const int32_t* neighbors, int32_t num_neighbors, int32_t redundancy, double* out, int32_t out_mem);

/* The scoring step of the RANSAC loop (registration.py:867-871, 958-969) for all hypotheses at once.  affines: n_hypotheses
 * row-major (ndim + 1)^2 fixed -> moving matrices; fixed / moving: n_corr x ndim candidate correspondences (all host memory).
 * count_out[h] = number of correspondences with || A_h f + t_h - m || <= max_error, sum_out[h] = the sum of those residuals (host
 * memory).  One wave per hypothesis: lane l adds correspondences l, l + 64, ... in order, the lanes are folded by a fixed shuffle
 * tree -- no floating-point atomics, equal inputs give equal bits. */
int mvs_marker_score(int device, const double* affines, int32_t n_hypotheses, const double* fixed, const double* moving,
                     int64_t n_corr, int32_t ndim, double max_error, int32_t* count_out, double* sum_out);

/* PSF extraction from beads (mv_deconv.extract_psf): the average of the background-subtracted, unit-sum windows around the beads of
 * one view, on the OUTPUT grid -- what mvs_mv_deconv takes as that view's forward kernel.  The reference has no counterpart; its
 * model, BigStitcher / multiview-reconstruction, measures the PSFs from the beads of the registration.
 *   view            uint8 / uint16 / float32, host (C-contiguous, staged as by mvs_resample) or device (stride[2] == 1); only
 *                   data / dtype / mem / shape / stride are read.  ndim 2: shape[0] == 1
 *   centers         host, n_beads x 3 (z, y, x; z = 0 in 2D): the beads in view pixel coordinates
 *   window_matrix   M, 3 x 3 row-major (2D: embedded like every matrix of this ABI): window offset o, in output-grid voxels, ->
 *                   view pixels; the window of a bead at c is c + M o for o in prod [-radius[k], radius[k]], x fastest
 *   radius          per axis, 1 .. MVS_PSF_MAX_RADIUS (the z entry is ignored in 2D)
 * Per bead, in double unless stated otherwise and without contraction:
 *   1. sample: s(o) = the view at ((M_k0 o_z + M_k1 o_y) + M_k2 o_x) + c_k, the linear sample of mvs_resample (float32).  A sample
 *      that is out of bounds (not 0 <= coordinate <= n - 1 on every axis) or NaN gives the bead status 1 (outside);
 *   2. background: bg = mean of s over the shell (|o_k| == radius[k] on some axis); e(o) = max(s(o) - bg, 0); sum e not a positive
 *      finite number: status 2 (empty);
 *   3. refine_iterations (0 .. 64) times: c += M (sum o e(o) / sum e), then 1-2 again at the new centre;
 *   4. u(o) = e(o) / sum e, kept as float32.
 * psf_out (host, the window's samples, x fastest) = (sum of u over the beads of status 0, in ascending bead index, float64) / their
 * number, as float32; all zero when no bead has status 0 (not an error: status_out says why).  stats_out[b] = (bg, sum e, the
 * Pearson correlation of u_b with psf_out over the window); NaN where a bead did not get that far.  centers_out[b] = the centre
 * the bead was last sampled at.  Every sum has a fixed order (a thread's strided samples in order, the lanes of a wave by shuffles,
 * the waves in order) and there are no floating-point atomics: equal inputs give equal bits.  The beads go through the kernels in
 * batches whose rows (window x 4 bytes per bead) fit a scratch budget; mvs_set_option "psf_batch" = n fixes the batch (0, the
 * default: automatic), and the result does not depend on it (with more than one batch the windows are gathered a second time for
 * the correlations).  Waits for the result; runs on the context lane of `device`. */
#define MVS_PSF_MAX_RADIUS 31
int mvs_psf_extract(int device, const mvs_view_t* view, int32_t ndim, const double* centers, int64_t n_beads,
                    const double window_matrix[9], const int32_t radius[3], int32_t refine_iterations, double* centers_out,
                    int32_t* status_out, float* stats_out, float* psf_out);

/* Tile intensity harmonisation (intensity.fit_maps / apply_maps): remove brightness steps between tiles (bleaching, light-sheet
 * side, detector offset, exposure) before fusion.  The reference has no counterpart.  Every view carries a grid of cells[] =
 * (gz, gy, gx) cells (2D: gz == 1), 1 .. MVS_INTENSITY_MAX_CELLS per axis, with a gain a and an offset b per cell.
 * THE CELL RULE, along an axis of n pixels with g cells (pixel centres at integer coordinates): the continuous coordinate c
 * belongs to cell clamp(floor((c + 0.5) * g / n), 0, g - 1), evaluated in double, the product before the quotient; the centre of
 * cell k is at (k + 0.5) * n / g - 0.5.
 *
 * mvs_intensity_pair_moments: the moments of mvs_pair_moments, split by the cells of both tiles.  fixed->matrix / offset and
 * moving->matrix / offset map a grid index to a pixel of the respective tile; halfspaces, dtypes (uint8 / uint16 / float32, one
 * for both views, else MVS_ERR_UNSUPPORTED), host / device memory and strided windows are as in mvs_pair_moments.  A record is a
 * box of the grid, lo[k] <= index[k] < lo[k] + n[k] (z, y, x; 2D: lo[0] == 0, n[0] == 1), plus one cell of each tile.  A voxel of
 * the box counts for the record iff
 *   - it passes steps 1-4 of mvs_pair_moments (mask, both samples in bounds and finite; the same device code), and
 *   - the cell rule puts its fixed pixel coordinate in cell_f and its moving pixel coordinate in cell_m on every axis.
 * Boxes therefore only need to be conservative: a sample belongs to exactly one (cell_f, cell_m) whatever boxes the host chose.
 * out (host memory) receives n_records rows of MVS_PAIR_MOMENTS_LEN doubles, (n, mean_f, mean_m, M2_f, M2_m, C_fm) of the
 * counted pairs (all six 0 when n == 0).  1 <= n_records <= MVS_INTENSITY_MAX_RECORDS; callers batch above that.
 * Launches: one for all records of the call -- record r owns min(max(ceil(voxels_r / MVS_INTENSITY_BLOCK_VOXELS), 1),
 * MVS_INTENSITY_MAX_BLOCKS) consecutive workgroups, a function of its own voxel count only; a prefix table built on the host maps
 * a workgroup to its record -- and a second one that folds each record's workgroup results.  Reduction as in mvs_pair_moments:
 * per thread an integer count and float64 sums shifted by its first counted pair, then the update of Chan, Golub and LeVeque in a
 * fixed tree (lanes by shuffles, waves through LDS, a record's workgroups in index order: each lane of one wave folds a run of
 * ceil(blocks / 64) consecutive ones, then the lanes merge).  No floating-point atomics and no completion counters; a record's
 * row does not depend on which other records share the call, and equal inputs give equal bits.  Waits for the result. */
#define MVS_INTENSITY_MAX_CELLS 16
#define MVS_INTENSITY_MAX_RECORDS 1024
#define MVS_INTENSITY_BLOCK_VOXELS 256
#define MVS_INTENSITY_MAX_BLOCKS 1024
typedef struct {
    int64_t lo[3], n[3];          /* box of the grid */
    int32_t cell_f[3], cell_m[3]; /* the cell of the fixed / moving tile */
} mvs_intensity_record_t;
int mvs_intensity_pair_moments(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int32_t ndim, const int32_t cells_f[3],
                               const int32_t cells_m[3], const double* halfspaces, int32_t n_halfspaces,
                               const mvs_intensity_record_t* records, int32_t n_records, double* out);

/* mvs_intensity_apply: out(p) = a(p) * view(p) + b(p) for every voxel of a tile.  Only data / dtype / mem / shape / stride of
 * `view` are read (uint8 / uint16 / float32; host C-contiguous, or device with stride[2] == 1).  coeff (host): (gz, gy, gx, 2)
 * float32, (a, b) per cell.  tables (host): for the axes z, y, x in turn, shape[k] int32 followed by shape[k] float32 -- per pixel
 * index the lower cell i of the two it lies between and the weight t of cell i + 1; the caller derives both in double from the
 * cell rule (coordinate clamped to the first and last cell centre; an axis with one cell: i = 0, t = 0), so the kernel divides
 * nothing.  The upper cell is min(i + 1, g - 1).
 * Arithmetic: float32 without contraction, lerp(u, v, t) = u + t * (v - u).  Per row (z, y) the gx coefficient pairs are
 * interpolated along z, then along y: lerp(lerp(c[z0][y0], c[z1][y0], tz), lerp(c[z0][y1], c[z1][y1], tz), ty); per voxel
 * a = lerp(a[x0], a[x1], tx), b likewise, then y = a * (float)I + b.  A float32 output stores y (a NaN input stays NaN); an
 * integer output stores rintf(y) (half to even) saturated to the type's range, a NaN as 0.
 * out: C-contiguous, shape of the view, in out_mem; out_dtype is the view's dtype or float32 (else MVS_ERR_UNSUPPORTED).  out may
 * be view->data itself for a contiguous device array with out_dtype == dtype (in place: every voxel is read once, by the lane that
 * writes it, before it is written).  One wave per row: the row's coefficient pairs in LDS, then 16-byte loads / stores per lane
 * along x (on the wider of the two element types) with a scalar head up to the row's first aligned element and a scalar tail; a
 * row whose input and output alignments differ goes element by element.  Waits for the result; runs on the lane of `device`. */
int mvs_intensity_apply(int device, const mvs_view_t* view, int32_t ndim, const int32_t cells[3], const float* coeff, const void* tables,
                        void* out, int32_t out_dtype, int32_t out_mem);

/* Shading (flat-field) correction (intensity.estimate_shading / apply_shading): remove the vignetting and uneven illumination that
 * every tile of an acquisition shares.  The reference has no counterpart.  The profile is estimated from a per-pixel order
 * statistic over the stack of all tiles and planes (mvs_stack_quantiles), smoothed and normalised on the host, and applied as a
 * per-pixel gain / offset plane (mvs_plane_apply).
 *
 * mvs_stack_quantiles: 1 <= n_views <= MVS_STACK_MAX_VIEWS tiles of one dtype (uint8 / uint16 / float32) and one (H, W) =
 * (shape[1], shape[2]); shape[0] may differ per view (2D: 1).  Only data / dtype / mem / shape / stride are read; stride[2] == 1,
 * stride[0] and stride[1] are arbitrary (windows, every k-th plane); host or device memory per view.  Anything else:
 * MVS_ERR_UNSUPPORTED.
 * THE SAMPLE SET of pixel (y, x) is view_v(z, y, x) over all v, z.  A float32 NaN is not a sample; +-inf are; -0 counts as +0.
 * n(y, x), the number of samples, goes to count_out (host, H x W int32); more than 2^31 - 1 planes in all are refused.
 * THE RANK RULE: out (host, n_q x H x W float32; 1 <= n_q <= MVS_STACK_MAX_QUANTILES, 0 <= q[j] <= 1) receives in out[j][y][x]
 * the sample of ascending 0-based rank floor((double)(n - 1) * q[j]), NaN where n == 0: numpy's quantile(..., method="lower")
 * (nanquantile for float32).  The result is a selection: exact, independent of the order of the views, of how planes are shared
 * among waves and workgroups and of host / device / window inputs; equal inputs give equal bits.
 * Algorithm (csrc/mvs_stack_select.h): most-significant-digit radix select with 8-bit digits on an order-preserving unsigned key
 * (the value itself for integers: 1 / 2 digits; for float32 the sign-flipped bit pattern, -0 first mapped to +0: 4 digits).  A
 * workgroup owns a strip of 128 bytes of one row (128 / 64 / 32 pixels; the last strip of a row may be shorter) for all samples
 * and keeps the strip's 256 bins per pixel as 32-bit counters in LDS (128 / 64 / 32 KiB; they cannot overflow); there are no
 * histograms in global memory.  Half a wave loads one plane's 128 bytes, 4 bytes per lane (element by element where the row is
 * not 4-byte aligned), and the 32 half waves of a workgroup take different planes of a device-side table of the views.  The top
 * digit is counted once for all quantiles, every further digit once per quantile over the samples that share the pixel's prefix:
 * the stack is read 1 + n_q * (digits - 1) times.  Integer LDS atomics only; no floating-point atomics.
 * Host views are packed into one device block of their total size for the duration of the call (pageable uploads at the rate
 * of the link, row by row for strided host windows): callers that ask more than once keep their tiles resident.
 * Waits for the result; runs on the context lane of `device`. */
#define MVS_STACK_MAX_VIEWS 4096
#define MVS_STACK_MAX_QUANTILES 4
int mvs_stack_quantiles(int device, const mvs_view_t* views, int32_t n_views, int32_t ndim, const double* q, int32_t n_q, float* out,
                        int32_t* count_out);

/* mvs_plane_apply: out(z, y, x) = a(y, x) * (float)view(z, y, x) + b(y, x).  view, out, out_dtype, out_mem, the float32
 * arithmetic without contraction, the rounding of integer outputs (rintf, saturated, a NaN stored as 0; a float32 output keeps
 * NaN) and in-place use are exactly those of mvs_intensity_apply.  coeff: (H, W, 2) float32, (a, b) per pixel, in coeff_mem =
 * host (uploaded by the call) or device memory (used in place: callers that correct many tiles upload once).
 * A wave takes one row y and a slab of planes; a lane keeps the coefficient pairs of its consecutive pixels in registers and walks
 * z, so the coefficient plane is read once per slab and not once per voxel.  16-byte loads / stores along x (on the wider of the
 * two element types) with a scalar head up to the row's first aligned element and a scalar tail; a row whose input and output
 * alignments differ, or change from plane to plane, goes pixel by pixel.  Waits for the result; runs on the lane of `device`. */
int mvs_plane_apply(int device, const mvs_view_t* view, int32_t ndim, const float* coeff, int32_t coeff_mem, void* out, int32_t out_dtype,
                    int32_t out_mem);

/* Non-rigid tile refinement (nonrigid.fit_fields / apply_fields): a local correction of what one affine per tile cannot describe
 * (stage non-linearity, field curvature, refractive distortion), between registration and fusion.  The reference has no
 * counterpart; BigStitcher's non-rigid fusion is the model.  Every view carries a grid of nodes[] = (gz, gy, gx) cells under THE
 * CELL RULE of the intensity maps (above; 2D: gz == 1; 1 .. MVS_FIELD_MAX_NODES per axis) with one displacement vector d per cell,
 * in pixels of that view, in axis order z, y, x.  The displacements are fitted on the host from the shifts that block matching
 * finds in the overlaps (mvs_block_match) and applied to whole tiles by mvs_field_warp.
 *
 * mvs_block_match: for every box ("block") of the overlap grid of a pair and every integer shift s of a search window, the six
 * moments of the sample pairs (f(g), m(g + s)), g in the block.  Views (uint8 / uint16 / float32, one dtype for both, else
 * MVS_ERR_UNSUPPORTED; host or device memory; strided windows with stride[2] == 1), halfspaces and the meaning of matrix / offset
 * (grid index -> pixel of the tile) are those of mvs_pair_moments.  A block is lo[k] <= index[k] < lo[k] + n[k] (z, y, x; 2D:
 * lo[0] == 0, n[0] == 1, radius[0] == 0).  0 <= radius[k] <= MVS_BLOCKMATCH_MAX_RADIUS and, per block, prod n + prod (n + 2 r) <=
 * MVS_BLOCKMATCH_MAX_FLOATS, else MVS_ERR_UNSUPPORTED.  1 <= n_blocks <= MVS_BLOCKMATCH_MAX_BLOCKS and n_blocks * S * 48 bytes <=
 * MVS_BLOCKMATCH_MAX_RESULT_BYTES, else MVS_ERR_INVALID_ARG: callers batch.
 * out (host memory): n_blocks * S * MVS_PAIR_MOMENTS_LEN doubles, S = prod (2 r_k + 1); the shift index runs z slowest and x
 * fastest, each axis from -r_k to r_k.  Row (block, s) = (n, mean_f, mean_m, M2_f, M2_m, C_fm) over the pairs (f(g), m(g + s)).  A
 * pair is counted iff every halfspace holds at g, the fixed coordinate of g is in bounds and f is finite, and the moving coordinate
 * of the integer grid point g + s is in bounds and m is finite (the halfspaces are not tested at g + s).  All six are 0 when n == 0.
 * Coordinates and samples follow the per-voxel rule of mvs_pair_moments (double, no contraction, float32 linear sample; the same
 * device code), so a moving sample depends on g + s only.
 * One workgroup of 4 waves per block.  Every sample of the block and of the block grown by r on every side is taken once and
 * kept in LDS (x fastest; NaN marks "not counted"); wave w takes the shifts w, w + 4, ...; for one shift lane l folds the block
 * voxels l, l + 64, ... in index order into sums shifted by its first counted pair, then the lanes merge by the update of Chan,
 * Golub and LeVeque in the fixed shuffle tree of mvs_pair_moments.  No atomics, no completion counters, no second launch; a
 * block's rows do not depend on the other blocks of the call and equal inputs give equal bits.  Waits for the result; runs on the
 * lane of `device`. */
#define MVS_BLOCKMATCH_MAX_RADIUS 8
#define MVS_BLOCKMATCH_MAX_FLOATS 15360   /* block + grown moving block in LDS: 60 KB, static */
#define MVS_BLOCKMATCH_MAX_BLOCKS 4096    /* per call; the wrapper batches, also so that the result stays <= 64 MiB */
#define MVS_BLOCKMATCH_MAX_RESULT_BYTES (64 << 20)
typedef struct { int64_t lo[3], n[3]; } mvs_block_t;
int mvs_block_match(int device, const mvs_view_t* fixed, const mvs_view_t* moving, int32_t ndim,
                    const double* halfspaces, int32_t n_halfspaces, const mvs_block_t* blocks,
                    int32_t n_blocks, const int32_t radius[3], double* out);

/* mvs_field_warp: out(p) = view(clamp(p + d(p), 0, n - 1)), read with the linear sampler of mvs_resample.  Only data / dtype / mem /
 * shape / stride of `view` are read (uint8 / uint16 / float32; host C-contiguous, or device with stride[2] == 1).  field (host):
 * (gz, gy, gx, 3) float32, (d_z, d_y, d_x) per cell, all finite (else MVS_ERR_INVALID_ARG); in 2D the z component is ignored
 * (taken as 0).  tables (host): the per-axis tables of mvs_intensity_apply (lower cell i and weight t of cell i + 1 per pixel
 * index; the upper cell is min(i + 1, g - 1)).
 * Arithmetic: d is interpolated in float32 without contraction, lerp(u, v, t) = u + t * (v - u), per component: per row (z, y)
 * along z, then along y -- lerp(lerp(d[z0][y0], d[z1][y0], tz), lerp(d[z0][y1], d[z1][y1], tz), ty) -- and per voxel along x.  The
 * coordinate is c_k = min(max((double)p_k + (double)d_k, 0), n_k - 1) per axis and the value the linear float32 sample at c with
 * all taps read (a NaN tap poisons a float32 sample; a zero field returns finite input bits).  A float32 output stores the value
 * (NaN stays NaN); an integer output stores rintf(value) (half to even) saturated to the type's range, a NaN as 0.
 * out: C-contiguous, shape of the view, in out_mem; out_dtype is the view's dtype or float32 (else MVS_ERR_UNSUPPORTED).  The
 * kernel gathers: when out overlaps the view's memory the call returns MVS_ERR_INVALID_ARG.  One wave per row, four rows per
 * workgroup: the row's gx displacement vectors in LDS, then every lane interpolates along x and gathers; stores of 16 bytes per
 * lane from the row's first 16-byte aligned output element on, with a scalar head and tail.  Waits for the result; runs on the
 * lane of `device`. */
#define MVS_FIELD_MAX_NODES 16
int mvs_field_warp(int device, const mvs_view_t* view, int32_t ndim, const int32_t nodes[3],
                   const float* field, const void* tables, void* out, int32_t out_dtype, int32_t out_mem);

/* Sample masks and mask-driven pair selection (masks.py): where the sample is, so that only the pairs of views whose sample masks
 * touch are registered.  Replaces registration.get_pairs_from_sample_masks (registration.py:3256-3292: fuse of mask_i * (i + 1) with
 * nanmin at order 0) and mv_graph.get_connected_labels (mv_graph.py:895-931) of the reference; the threshold is one Otsu threshold
 * for the whole acquisition, from one histogram over all tiles.  All four results are integers or selections: integer atomics
 * only, no floating-point atomics, equal inputs give equal bits.  All four wait for the result and run on the context lane of
 * `device`.
 *
 * mvs_tile_histogram: over n_tiles >= 1 tiles of one dtype (uint8 / uint16 / float32, else MVS_ERR_UNSUPPORTED) whose shapes may
 * differ.  Only data / dtype / mem / shape / stride are read; stride[2] == 1; device tiles may be strided windows, host tiles are
 * C-contiguous (packed into one device block for the duration of the call); rows of at most 2^29 voxels.
 * n_bins == 0: *min_out, *max_out and *n_valid_out receive minimum, maximum and number of the voxels that are not NaN (min / max:
 * NaN when there is none): per-workgroup partials and a second small launch.
 * 1 <= n_bins <= MVS_HIST_MAX_BINS (above: MVS_ERR_UNSUPPORTED): counts_out (host, n_bins uint64) receives the counts of
 * numpy.histogram(values.astype(float64), bins=n_bins, range=(lo, hi)) over all tiles together, exactly.  edges (host): numpy's own
 * n_bins + 1 float64 edges, lo = edges[0] < hi = edges[n_bins].  THE INDEX RULE, in float64 without contraction: a NaN and a value
 * outside [lo, hi] are not counted; k = trunc((v - lo) / (hi - lo) * n_bins); k == n_bins becomes n_bins - 1; one step down when
 * v < edges[k], else one step up when v >= edges[k + 1] and k is not the last bin.
 * A wave takes one row of one tile: 16-byte loads from the row's first 16-byte aligned element on, a scalar head and tail.  A
 * workgroup counts into uint32 bins in LDS (LDS integer atomics; the grid is sized so that a workgroup sees fewer than 2^32 voxels)
 * and flushes them once with global uint64 integer atomics. */
#define MVS_HIST_MAX_BINS 4096
int mvs_tile_histogram(int device, const mvs_view_t* tiles, int32_t n_tiles, int32_t n_bins, const double* edges, uint64_t* counts_out,
                       double* min_out, double* max_out, int64_t* n_valid_out);

/* mvs_mask_threshold: mask_out (device memory, uint8, C-contiguous, the tile's shape) = 1 where tile > threshold, else 0.  tile:
 * uint8 / uint16 / float32 in device memory, stride[2] == 1 (only data / dtype / mem / shape / stride are read).  An integer voxel is
 * compared exactly, (double)v > threshold; a float32 voxel against (float)threshold; a NaN gives 0.
 * radius[] (z, y, x; 2D: radius[0] ignored), 0 <= radius[k] <= MVS_MASK_MAX_DILATE (above: MVS_ERR_UNSUPPORTED): the mask is then
 * dilated by the flat box of 2 radius[k] + 1 voxels per axis, scipy.ndimage.maximum_filter(mask, size=2 r + 1, mode="constant",
 * cval=0), as separable line passes x, y, z on uint8 work volumes whose rows start on 16-byte boundaries.  Every lane takes 16
 * voxels: the x pass reads the 16-byte groups around its own as bits and ORs a window of 2 r + 1 bits by doubling, the y / z passes
 * OR the 16-byte groups of the 2 r + 1 rows / planes.  *n_set_out (may be NULL): the number of set voxels of mask_out. */
#define MVS_MASK_MAX_DILATE 32
int mvs_mask_threshold(int device, const mvs_view_t* tile, int32_t ndim, double threshold, const int32_t radius[3], void* mask_out,
                       int64_t* n_set_out);

/* mvs_label_fuse: the reference's fuse(mask_i * (i + 1), fusion_func=nanmin, interpolation_order=0) followed by its nan_to_num, on
 * one output grid.  views: n_views >= 1 uint8 masks (else MVS_ERR_UNSUPPORTED), host (C-contiguous) or device memory (stride[2] ==
 * 1); matrix / offset map an index of the output grid to a pixel of the view, as for mvs_fuse_chunk (fusion.fuse_np's
 * get_pixel_affines derivation; the weight fields are not read).  out: int32, out_shape (z, y, x; 2D: out_shape[0] == 1),
 * C-contiguous, in out_mem.  Per output voxel p and every view v whose coordinate is in bounds (0 <= c <= n - 1 on every axis, in
 * float64 without contraction, as mvs_resample tests it) the value is mask_v(floor(c + 0.5)) ? v + 1 : 0 -- the voxel mvs_resample
 * picks at order 0 -- and out(p) their minimum, zeros included; 0 where no view covers p.  Bricks of 4 x 4 x 64 (2D: 16 x 64) voxels;
 * a workgroup culls the views against its brick, 64 at a time, as the generic fuse kernel does: any number of views. */
int mvs_label_fuse(int device, const mvs_view_t* views, int32_t n_views, int32_t ndim, const int64_t out_shape[3], int32_t* out,
                   int32_t out_mem);

/* mvs_label_contacts: which labels touch (mv_graph.py:895-931).  labels: int32, device memory, C-contiguous, shape (z, y, x; 2D:
 * shape[0] == 1); values outside 1 .. n_labels count as background.  1 <= n_labels <= MVS_LABEL_MAX (above: MVS_ERR_UNSUPPORTED; the
 * matrix is at most 32 MiB).  counts_out (host): n_labels x n_labels uint64; C[a - 1][b - 1], a < b, is the number of voxel pairs
 * (p, p + o) with labels {a, b}, o over the half neighbourhood of `connectivity` = the number of axes that may differ, 1 .. ndim:
 * the offsets in {-1, 0, 1}^ndim with at most that many non-zero components whose first non-zero component is +1 -- 2 / 4 offsets in
 * 2D, 3 / 9 / 13 in 3D, anti-diagonals such as (+1, -1) included.  Everything else of the matrix is 0.  (The reference compares the
 * +1 shifts along one axis in 2D, one or two axes in 3D, and lists ordered pairs.)
 * A wave takes 64 consecutive voxels of a row; per offset, consecutive lanes with the same label pair are combined by one shuffle and
 * one ballot and the first lane of the run adds its length with one global uint64 integer atomic. */
#define MVS_LABEL_MAX 2048
int mvs_label_contacts(int device, const int32_t* labels, int32_t ndim, const int64_t shape[3], int32_t n_labels, int32_t connectivity,
                       uint64_t* counts_out);

/* Stitching per-tile segmentations (labels.py): one int32 label tile per view, with ids that mean nothing outside their tile, becomes
 * one label image.  The voxel count of every label (mvs_label_counts) and the co-occurrence table of the labels of every pair of
 * overlapping tiles (mvs_label_pair_overlaps) go to the host, which matches labels across tiles and numbers the objects
 * (labels.match_labels, float64); mvs_label_tiles_fuse then paints every view's labels through its look-up table.
 * LABEL TILES are int32 BY CONTRACT: mvs_view_t.dtype is not read (enum mvs_dtype has no code for them and the image entry points
 * keep refusing them).  Host tiles are C-contiguous and staged for the duration of the call; device tiles have stride[2] == 1 and
 * may be strided windows; data is aligned to 4 bytes; 2D: shape[0] == 1.  A negative label is background (0).
 * COORDINATES are float64 without contraction in the operation order of the sampler, c_k = ((M_k0 p_z + M_k1 p_y) + M_k2 p_x) + o_k.
 * A tile is IN BOUNDS at p when 0 <= c_k <= n_k - 1 on every axis, and its voxel is q = floor(c + 0.5): the rule of mvs_resample /
 * mvs_label_fuse at order 0.
 * Integer atomics only: equal inputs give equal results (the triples of a table: after sorting).  All three wait for their result
 * and run on the context lane of `device`.
 *
 * mvs_label_counts: counts_out (host, `capacity` uint64) receives n[l] = the number of voxels of `tile` with max(label, 0) == l, for
 * l = 0 .. capacity - 1; only data / mem / shape / stride of the tile are read.  *max_label_out: the largest max(label, 0) of the
 * tile.  A label >= capacity is not counted and is no error: the caller looks at *max_label_out and calls again with capacity =
 * max + 1.  1 <= capacity <= MVS_LABEL_COUNT_MAX_CAPACITY (below: MVS_ERR_INVALID_ARG, above: MVS_ERR_UNSUPPORTED).
 * A wave takes 64 consecutive voxels of a row at a time -- where they are whole and 16-byte aligned, as sixteen 16-byte loads handed
 * out by shuffles -- and a contiguous range of such chunks in all.  Equal labels of consecutive lanes are combined by one shuffle
 * and one ballot and the first lane of the run adds its length with one global uint64 integer atomic (the scheme of
 * mvs_label_contacts); a chunk of ONE label is carried in registers into the next chunks while the label stays, so background and
 * the inside of large objects cost one atomic per wave. */
#define MVS_LABEL_COUNT_MAX_CAPACITY 2147483648LL
int mvs_label_counts(int device, const mvs_view_t* tile, int32_t ndim, int64_t capacity, uint64_t* counts_out, int64_t* max_label_out);

/* mvs_label_pair_overlaps: the co-occurrence table of ONE directed pair of label tiles (a, b).  b->matrix / b->offset map a pixel
 * index of a to a pixel coordinate of b (transformation.get_pixel_affine with a's grid as the output grid); of a only data / mem /
 * shape / stride are read.  For every voxel p of the box [box_lo, box_lo + box_n) of a (inside a, not empty, else
 * MVS_ERR_INVALID_ARG; the caller passes a box that bounds b's footprint, and every voxel of it is still tested) at which b is in
 * bounds, with la = max(A[p], 0) and lb = max(B[q], 0): when la | lb is not 0 the entry (la, lb) of the table counts one.  Rows with
 * one zero label are part of the table: they carry the marginals.
 * OUT: *n_unique_out = the number of entries of the table; la_out / lb_out (host, int32) and n_out (host, uint64), `capacity` each,
 * receive min(n_unique, capacity) triples (la, lb, count) in NO DEFINED ORDER: the caller sorts.  Returns MVS_OK when the triples
 * are the whole table and MVS_LABEL_INCOMPLETE (positive: not an error, mvs_last_error is not set) when n_unique > capacity; the
 * caller calls again with a capacity >= n_unique.  1 <= capacity <= MVS_LABEL_PAIR_MAX_CAPACITY.
 * THE TABLE is open addressing in device scratch of the call: the 64-bit key la << 32 | lb, the power of two >= 2 * capacity (at
 * least 1024) slots of a uint64 key and a uint64 count, the first slot from the splitmix64 finaliser of the key, linear probing.
 * An insertion is a lock-free compare-and-swap EMPTY -> key on the slot's key followed by an integer add on its count.  PROBING IS
 * BOUNDED by the number of slots: with the table exhausted -- more entries than slots -- the voxel is dropped and a flag raised; the
 * call then also returns MVS_LABEL_INCOMPLETE, *n_unique_out is the number of slots (a lower bound of the table's size, above
 * capacity) and the counts of the triples are not to be used.  No lane waits for another one: no locks, no spinning on a flag.
 * A wave takes 64 consecutive voxels of a row of the box at a time; equal pairs of consecutive lanes are combined before they touch
 * the table, and a chunk of one pair is carried in registers as in mvs_label_counts.  A second small launch compacts the occupied
 * slots, one integer atomic per wave. */
#define MVS_LABEL_PAIR_MAX_CAPACITY 134217728LL
#define MVS_LABEL_INCOMPLETE 1
int mvs_label_pair_overlaps(int device, const mvs_view_t* a, const mvs_view_t* b, int32_t ndim, const int64_t box_lo[3],
                            const int64_t box_n[3], int64_t capacity, int32_t* la_out, int32_t* lb_out, uint64_t* n_out,
                            int64_t* n_unique_out);

/* mvs_label_tiles_fuse: the label image of n_views >= 1 label tiles on one output grid.  views[i].matrix / offset map an index of
 * the FRAME -- the whole output grid -- to a pixel of view i, as for mvs_label_fuse; the output is the box of out_shape (z, y, x;
 * 2D: out_shape[0] == 1) voxels whose first voxel has the frame index index_origin (NULL: zeros).  The indices are shifted as
 * integers, as the index frame of mvs_fuse_opts_t does, so a box equals the crop of the whole grid's result bit for bit.
 * luts (NULL: every view the identity): per view a pointer into DEVICE memory to lut_len[i] >= 1 int32 entries, or NULL for the
 * identity.  out: int32, C-contiguous, in out_mem.
 * Per output voxel p, among the views in bounds, the winner w is the one with the largest d_v = min over the axes with n_k > 1 of
 * min(c_k, (n_k - 1) - c_k) -- the interior-most view decides -- and ties go to the lowest view index.  out(p) = lut_w[L_w(q)], and 0
 * when that label is negative or >= lut_len[w] (the identity has no upper limit) or no view is in bounds.  The winner's background
 * wins too: seams are hard.
 * Bricks of 4 x 4 x 64 (2D: 16 x 64) voxels; a workgroup culls the views against its brick, 64 at a time, as mvs_label_fuse does:
 * any number of views. */
int mvs_label_tiles_fuse(int device, const mvs_view_t* views, int32_t n_views, int32_t ndim, const int32_t* const* luts,
                         const int64_t* lut_len, const int64_t out_shape[3], const int64_t index_origin[3], int32_t* out, int32_t out_mem);

/* mvs_label_components: the connected components of one thresholded tile, numbered as scipy.ndimage.label numbers them -- the step
 * between a mask (mvs_mask_threshold) and the label tiles the entries above stitch.  `tile` is an IMAGE tile: UNLIKE the other label
 * entries its dtype is read (uint8, uint16 or float32; else MVS_ERR_UNSUPPORTED).  Host tiles are C-contiguous and staged for the
 * duration of the call; device tiles have stride[2] == 1 and may be strided windows; 2D: shape[0] == 1; only data / dtype / mem /
 * shape / stride are read.  At most 2^31 - 1 voxels (above: MVS_ERR_UNSUPPORTED).
 * FOREGROUND is (float)v > threshold: a voxel equal to the threshold and a NaN are background; a uint8 mask is labelled with
 * threshold = 0.  NEIGHBOURHOOD: connectivity 1 .. ndim (else MVS_ERR_INVALID_ARG) is that of scipy.ndimage.
 * generate_binary_structure(ndim, connectivity) -- the offsets in {-1, 0, 1}^ndim with at most `connectivity` non-zero components,
 * whose half has the 2 / 4 (2D) and 3 / 9 / 13 (3D) offsets of mvs_label_contacts.
 * OUT: labels_out, int32, C-contiguous, of the tile's shape, in out_mem: 0 at background; the components with at least min_voxels
 * voxels carry the ids 1 .. n in ascending raster order of their first voxel (the numbering of scipy.ndimage.label), smaller ones
 * are 0; min_voxels <= 1 keeps everything.  *n_labels_out = n.
 * Launches: rows (a wave takes 64 consecutive voxels of a row at a time, 16-byte loads where they are whole and aligned, and writes
 * per voxel the index of the first voxel of its run of foreground along x, carried across chunks), merge (per offset with a y or z
 * component the first lane of every run of touching voxels joins the two runs by a lock-free union: find both roots, atomic minimum
 * of the smaller into the larger one's parent, go on from the returned value when that one was no root any more), flatten (every
 * voxel to its root; with min_voxels > 1 also the voxels per root, runs combined before the atomic as in mvs_label_counts), the
 * numbering of the roots by an exclusive scan in raster order as three launches (counts per workgroup, one workgroup over the
 * counts, ranks at the roots; no workgroup waits for another one), relabel.  A parent index is never above its voxel's own and is
 * only ever lowered, so every chase ends and the root of a component is its first voxel in raster order whatever the order of
 * execution.  Integer atomics only: equal inputs give equal bits.  The call waits for its result and runs on the context lane of
 * `device`.  Scratch of the context's allocator: 4 bytes per voxel, 4 more with min_voxels > 1, 8 KiB for the scan; a host tile and
 * a host result are staged next to it. */
int mvs_label_components(int device, const mvs_view_t* tile, int32_t ndim, float threshold, int32_t connectivity, int64_t min_voxels,
                         int32_t* labels_out, int32_t out_mem, int64_t* n_labels_out);

/* Masks as fusion weights (masks.feather, fuse(view_weights=)): a binary mask becomes a feathered uint8 weight tile, and the
 * weighted chunk entry takes one such tile per view next to the image.
 *
 * mvs_mask_feather: out (uint8, C-contiguous, the mask's shape, in out_mem) = W(p) = rint(252 (1 - cos(pi min(t, 1))) / 2), with
 *   t^2 = min over the ZERO voxels q of the mask of sum_k ((p_k - q_k) / width[k])^2.
 * mask: uint8, nonzero = use; host (C-contiguous; staged for the duration of the call) or device memory (stride[2] == 1; may be a
 * strided window); only data / dtype / mem / shape / stride are read.  width[] (z, y, x; 2D: width[0] ignored): the feather width
 * per axis in voxels, 1 <= width[k] <= MVS_FEATHER_MAX_WIDTH (below: MVS_ERR_INVALID_ARG, above: MVS_ERR_UNSUPPORTED).  Voxels
 * outside the array do not count as zero; a zero voxel gives 0; a mask without a zero gives MVS_FEATHER_FULL_WEIGHT everywhere; with
 * every width 1 the result is 0 / 252 (no feather).
 * WHAT IS EXACT.  D = prod_k width[k]^2 <= 2^30 and P_k = D / width[k]^2 are integers, and N(p) = min(D, min_q sum_k (p_k - q_k)^2
 * P_k) = D min(t, 1)^2 is computed exactly in uint32 by separable min-plus passes: x (the nearest zero of the row within the width,
 * from the zero voxels of 80 positions as bits), then y, then z (min over |j| <= width of N_prev(p + j e_k) + j^2 P_k, capped at D
 * after every pass; a capped value plus one term is at most 2^31).  The last pass forms W = rint(252 (0.5 (1 - cos(pi sqrt((double)N /
 * D))))) in float64, to nearest even; N == 0 and N == D give 0 and 252 without the cosine.  At t = 0, 1/3, 1/2, 2/3, 1 -- the only
 * rational t with a rational cosine -- 252 times the ramp is an integer, so no exact tie reaches the rounding; a voxel whose value
 * before rounding lies within an ulp of a half-integer may differ by one from another libm.  Integer minima in a fixed order, no
 * atomics: equal inputs give equal bytes.
 * MEMORY.  The passes run in z slabs with a halo of width[0] planes: two uint32 plane sets of (planes + 2 width[0]) ny nx voxels in
 * device scratch, at most 256 MiB together unless one plane with its halo needs more.  mvs_set_option "feather_slab_planes" = n
 * fixes the output planes per slab (0, the default: sized to that budget); the result does not depend on it.  Waits for the result;
 * runs on the context lane of `device`. */
#define MVS_FEATHER_MAX_WIDTH 32
#define MVS_FEATHER_FULL_WEIGHT 252
int mvs_mask_feather(int device, const mvs_view_t* mask, int32_t ndim, const int32_t width[3], void* out, int32_t out_mem);

/* mvs_fuse_chunk_weighted: mvs_fuse_chunk through the generic (full affine map per voxel) kernel with a weight tile per view.
 * views, opts, out: as for mvs_fuse_chunk (index frame and index_offset included); opts->weights other than MVS_WEIGHTS_NONE is
 * MVS_ERR_UNSUPPORTED.  wviews[i]: the weight tile of view i -- uint8, host (C-contiguous) or device memory (stride[2] == 1), with
 * its own shape, stride, matrix and offset (a tile may live on a coarser grid than the image; matrix / offset map an index of the
 * frame to a pixel of the tile); always the WHOLE tile: index_offset must be 0.  data == NULL: the view has no weights (m = 1).
 * Only data / dtype / mem / shape / stride / matrix / offset / index_offset of a weight tile are read.
 * Per output voxel p (chunk index + opts->index_origin), views in view order:
 *   1. the image sample s_v, the in-bounds test and, under weighted average, the blend weight b_v, with the bits the generic kernel
 *      of mvs_fuse_chunk gives them (float64 coordinates without contraction, float32 interpolation);
 *   2. m_v = the linear sample of the tile / 252 as a float32: the coordinate clamped per axis into [0, n - 1] (scipy's
 *      mode="nearest"), a stored value above 252 counted as 252, lerp(u, v, t) = u + t (v - u) along x, then y, then z (exact where
 *      the taps are equal: an all-252 tile gives exactly 1), one division by 252 -- all in float64, the coefficients being
 *      differences of float64 coordinates -- and one rounding to float32.  (A float32 coefficient of a coordinate an integer -+ 1e-10
 *      is 0 or 1; step 3 would then see a tile edge differently from scipy's float64 sum.);
 *   3. view v takes part iff it is in bounds, s_v is not NaN and m_v > 0;
 *   4. weighted average: sum (b_v m_v) s_v / sum (b_v m_v) over the views that take part, accumulated in view order in float32 with
 *      the single-view state of the generic kernel (one view: s_v itself), 0 where the sum of weights is 0; max and simple average:
 *      over the views that take part; 0 where none does;
 *   5. nan_to_num, the halo trim and the truncating cast of mvs_fuse_chunk.
 * Views are culled per brick of 4 x 4 x 64 (2D: 16 x 64) voxels in view order, so the float32 sums have one order whatever the
 * chunking.  With every m_v == 1 a voxel goes through the float32 operations of the generic kernel in the same order: the result has
 * the bits of mvs_fuse_chunk under option "force_generic".  uint8 / uint16 / float32, 2D and 3D, any number of views.  Counter
 * "fuse_weighted_chunks" counts the chunks; the family counters of mvs_fuse_chunk stay untouched.  A host result is waited for; a
 * device result is waited for only when host slabs or tiles were staged. */
int mvs_fuse_chunk_weighted(int device, const mvs_view_t* views, const mvs_view_t* wviews, int32_t n_views, const mvs_fuse_opts_t* opts,
                            void* out);

/* Masked normalised cross-correlation of two overlap crops (registration.masked_correlation_registration): Padfield 2012, what
 * skimage.registration.phase_cross_correlation computes when it is given reference_mask / moving_mask.  The reference only ever calls
 * that variant with inverted masks (registration.py:433-443), where it contributes t = 0; this entry is the variant itself.
 *
 * THE CONTRACT.  Crops F (fixed) and M (moving): float32, C-contiguous, one shape n = (z, y, x) (2D: shape[0] == 1), in opts->mem.
 * A voxel of F is valid when it is finite, fixed_mask (uint8, the crop's shape, in opts->mask_mem; may be NULL) is non-zero there and,
 * with has_valid_above[0], (double)F(x) > valid_above[0]; likewise M with moving_mask and index 1.  For every integer shift s of the
 * window |s_d| <= S_d (S_d = max_shift[d]; n_d - 1 where that is negative or larger):
 *   Omega(s) = {x : F valid at x, x + s inside the crop, M valid at x + s},  N(s) = |Omega(s)|,
 *   r(s) = the Pearson correlation of F(x) and M(x + s) over Omega(s); 0 where sqrt(dF dM) <= 1e3 FLT_EPSILON max_s sqrt(dF dM) (the
 *          rule of skimage at float32), dF and dM the sums of squared deviations of either crop over Omega(s); clipped to [-1, 1].
 * A shift is eligible when N(s) >= max(overlap_ratio * max_s N(s), min_overlap), both maxima over the window.  The result is the
 * eligible shift with the largest r, among equals the one with the lowest flat index of the window (first axis slowest, s ascending):
 * M(x + peak) ~ F(x), the convention of the other pair functions.
 *
 * THE CHAIN, one stream, no host step in the middle.  Padded length per axis P_d = the smallest power of two >= n_d + S_d (1 where
 * n_d == 1): the circular correlation is then alias-free on the window.  prod(P) > MVS_MASKED_CORR_MAX_VOXELS is refused with
 * MVS_ERR_UNSUPPORTED before any device is touched (three complex64 volumes of prod(P): 6.4 GB at the limit); a lower max_shift is
 * the way out.  Statistics: count, sum (float64), min, max of the valid voxels per crop, per-workgroup partials and a second small
 * launch; mu = sum / count, range = max - min (1 where 0).  Pack: Z1 = f + i g, Z2 = vF + i vM, Z3 = f^2 + i g^2, zero-padded, with
 * f = (F - mu_F) / range_F on valid voxels and 0 elsewhere (r is invariant to both; the centring keeps the sums below out of float32
 * cancellation).  Three forward transforms (the transform of mvs_fft_c2c).  One combine kernel separates the six real spectra by
 * A(k) = (Z(k) + conj Z(-k)) / 2, B(k) = (Z(k) - conj Z(-k)) / 2i and forms, in place and scaled by 1 / prod(P),
 * X1 = corr(vF, vM) + i corr(f, g), X2 = corr(f, vM) + i corr(vF, g), X3 = corr(f^2, vM) + i corr(vF, g^2) with
 * corr(a, b)(s) = sum_x a(x) b(x + s), spectrum conj(A) B; one thread owns the pair {k, -k mod P}.  Three inverse transforms.  Over
 * the window only (at the wrapped indices): (a) the maxima of rint(N) and of sqrt(dF dM), dF = cF2 - cF^2 / N clamped at 0, N taken
 * as max(rint(N), 1); (b) r = (cFM - cF cM / N) / sqrt(dF dM) under the rule above, eligibility on rint(N), the arg-max per
 * workgroup; then one workgroup folds those and writes the record.  Fixed-tree reductions and no atomics: equal inputs give equal bits.
 *
 * r_out / n_out (host memory, may be NULL): the window's r (float32) and rint(N) (int32), shape (2 S_z + 1, 2 S_y + 1, 2 S_x + 1).
 * A status other than MVS_MASKED_CORR_OK is not an error (the call returns 0): TOO_FEW_VALID (a crop with fewer than min_overlap
 * valid voxels) before CONSTANT_CROP (min == max over a crop's valid voxels) before NO_ELIGIBLE_SHIFT (no eligible shift whose
 * denominator is above the tolerance); peak and r are then not to be used (with no eligible shift at all: peak 0, r NaN). */
#define MVS_MASKED_CORR_MAX_VOXELS (1LL << 28)
enum mvs_masked_corr_status {
    MVS_MASKED_CORR_OK = 0,
    MVS_MASKED_CORR_NO_ELIGIBLE_SHIFT = 1,
    MVS_MASKED_CORR_TOO_FEW_VALID = 2,
    MVS_MASKED_CORR_CONSTANT_CROP = 3
};
typedef struct mvs_masked_corr_opts_t {
    int32_t ndim;               /* 2 or 3                                              */
    int32_t mem;                /* enum mvs_mem of both crops                          */
    int32_t mask_mem;           /* enum mvs_mem of the masks that are given            */
    int32_t has_valid_above[2]; /* fixed, moving                                       */
    int32_t reserved;
    double valid_above[2];
    double overlap_ratio;       /* in (0, 1]                                           */
    int64_t min_overlap;        /* >= 1                                                */
    int64_t max_shift[3];       /* z, y, x; negative: n - 1                            */
} mvs_masked_corr_opts_t;
typedef struct mvs_masked_corr_result_t {
    int32_t status;             /* enum mvs_masked_corr_status                         */
    int32_t peak[3];            /* z, y, x                                             */
    float r;                    /* at the peak                                         */
    int32_t reserved;
    int64_t n_peak;             /* N at the peak                                       */
    int64_t n_max;              /* max N over the window                               */
    int64_t n_valid[2];         /* valid voxels of the fixed and of the moving crop    */
    float neighbour_r[6];       /* r at peak - e_d ([2 d]) and peak + e_d ([2 d + 1]); NaN outside the window */
    int32_t neighbour_ok[6];    /* ... inside the window and eligible                  */
    int64_t padded[3];          /* P                                                   */
    int64_t max_shift[3];       /* S                                                   */
} mvs_masked_corr_result_t;
int mvs_masked_corr(int device, const float* fixed, const float* moving, const uint8_t* fixed_mask, const uint8_t* moving_mask,
                    const int64_t shape[3], const mvs_masked_corr_opts_t* opts, mvs_masked_corr_result_t* result, float* r_out,
                    int32_t* n_out);

#ifdef __cplusplus
}
#endif
#endif /* MVS_HIP_H */
