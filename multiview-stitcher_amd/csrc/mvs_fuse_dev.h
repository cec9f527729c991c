// mvs_fuse_dev.h -- internal: device-side view record of the generic fuse path and launch helpers
// shared between mvs_fuse.hip and mvs_gauss.hip.
#pragma once
#include "mvs_internal.h"

struct DevView {
    const void* data;
    long long stride_z, stride_y;   // elements
    int nz, ny, nx;                 // slab shape
    int wnz;                        // z extent of the support table: 5 (3D) or 1 (2D)
    double m[9];
    double off[3];
    double wm[9];
    double woff[3];
    float edt[125];
    // ---- translation fast path (valid when tr_ok): matrix == I, diagonal support map; set by prepare_translation_view
    // (mvs_fuse_chunk_plan.h) ----
    int tr_ok;
    int io[3];        // input index = chunk index + io
    float fw[3];      // fractional interpolation weights (0 => single tap on that axis)
    int lo[3], hi[3]; // chunk-index range where the view is in bounds, exact per scipy's test
    float ws[3];      // tent scales of the closed-form support table edt = min_d(ws_d * tent(i_d))
    float sup_k[3];   // support nodes per output pixel (= w_matrix diagonal)
    // chunk-index coordinates of support nodes 0 and 4, split as ilo + flo and ihi - fhi with
    // integer ilo/ihi and fractions in [0,1): distances to them are exact in float
    int sup_ilo[3], sup_ihi[3];
    float sup_flo[3], sup_fhi[3];
    long long span;   // elements from data[0] to the last voxel of the slab, + 1
    float pad[3];     // pad[0]: 1 = linear interpolation (set with tr_ok)
};

// Device record of a view's weight tile (mvs_fuse_chunk_weighted): uint8, the whole tile on a grid of its own.  data == NULL: the
// view has no weights (1 everywhere).  m / off map a chunk index to a pixel of the tile (fill_weight_view, mvs_fuse_chunk_plan.h).
struct WeightView {
    const unsigned char* data;
    long long stride_z, stride_y;   // bytes
    int nz, ny, nx;
    int pad;
    double m[9];
    double off[3];
};

// ---- the prologue the chunk entries share (mvs_fuse.hip) ----
// what every entry requires of (views, opts, out); `what` = the entry's name, the prefix of the messages
int mvs_check_chunk_args(MvsContext* c, const char* what, const mvs_view_t* views, int32_t n_views, const mvs_fuse_opts_t* opts, const void* out);
// host slabs of the views: check them and size the device area they go through (the caller's choice: scratch slot 0, or part of
// its own work block) ...
int mvs_stage_views_bytes(MvsContext* c, const mvs_view_t* views, int n_views, size_t es, size_t* bytes);
// ... then, per view, queue its upload at area + *cursor; *dev_data = where the kernels read the view (v.data for a device view)
int mvs_stage_view(MvsContext* c, const mvs_view_t& v, size_t es, char* area, size_t* cursor, const void** dev_data);

// the record of a view that reads its data at dev_data (checks the x stride and the shape; the fill itself: mvs_fuse_chunk_plan.h)
int mvs_fill_dev_view(MvsContext* c, const mvs_view_t& v, int ndim, const void* dev_data, DevView* d);

// ---- the prologue of the entries that take one or two whole tiles (metrics, PSF extraction, intensity, shading, mvs_resample) ----
// what they require of a tile: data, a known mem and dtype, one plane in 2D; `what` = the entry's name.  Needs no device: `c` may
// be the context of mvs_ctx(device) before mvs_check_ready.
int mvs_check_tile_view(MvsContext* c, const char* what, const mvs_view_t* v, int ndim);
// the n (1 or 2) checked tiles through scratch slot 0: sizes the slot and queues the uploads of the host tiles.  Where the kernels
// read tile i goes to dev_data[i] and, with mvs_fill_dev_view and no translation path, into *dviews[i]; either array may be NULL.
int mvs_stage_tile_views(MvsContext* c, const mvs_view_t* const* views, int n, int ndim, const void** dev_data, DevView* const* dviews);

// `box0` (may be null): chunk index of the output array's first voxel -- the output is a sub-box of the chunk, evaluated with the
// chunk's own coordinates
void mvs_launch_resample(MvsContext* c, const DevView& d, int dtype, int order, float cval, float* out, const int64_t shape[3], const int* box0 = nullptr,
                         MvsCropStats* crop_stats = nullptr, int crop_stats_k = 0);
void mvs_launch_blend(MvsContext* c, const DevView& d, float* out, const int64_t shape[3], const int* box0 = nullptr);
// both for the boxes of up to 8 views in two launches (`dviews`: the same records in device memory)
// (`tr`: the views' translation-path records, or NULL -- with them the blend weights come from the closed form in float arithmetic)
struct TrView;
void mvs_launch_boxes_batch(MvsContext* c, const DevView* hviews, const DevView* dviews, int n_views, int dtype, int order, float cval,
                            float* const* res_out, float* const* blend_out, const int64_t (*shapes)[3], const int (*box0)[3],
                            const TrView* tr = nullptr);
// the translation-path kernel families of a chunk (mvs_fuse_region.hip, mvs_fuse_rows.hip); *done: the family took the chunk
int mvs_fuse_regions(MvsContext* c, const TrView* htr, const TrView* dtr, int n_views, int dtype, void* dout, const int64_t os[3],
                     const int64_t trim[3], bool* done);
int mvs_fuse_rows(MvsContext* c, const TrView* htr, const TrView* dtr, int n_views, int dtype, void* dout, const int64_t os[3],
                  const int64_t trim[3], bool* done);
// The host arithmetic on these records -- the translation-path constants (tr_view_in_chunk), the chunk frame (view_to_chunk_frame) and
// the chunk box (view_chunk_box) -- is mvs_fuse_chunk_plan.h's.
