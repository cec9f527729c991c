"""Shared helpers of the parity tests: build the same chunk inputs for the oracle and the HIP path."""
import numpy as np
from scipy import ndimage

from oracle import fuse_oracle as fo
from oracle import reg_oracle as ro


class SignedView:
    """torch's __cuda_array_interface__ import has no uint16: hand a DeviceArray's bytes over as int16 (the test mosaics stay below 4096)."""

    def __init__(self, arr):
        self.__cuda_array_interface__ = dict(arr.__cuda_array_interface__, typestr="<i2")
        self.owner = arr


def sim_to_view(sim):
    from multiview_stitcher_amd import spatial_image_utils as si

    sdims = si.get_spatial_dims_from_sim(sim)
    o, s = si.get_origin_from_sim(sim, asarray=True), si.get_spacing_from_sim(sim, asarray=True)
    return {"data": np.asarray(sim.data), "origin": o, "spacing": s}, fo.bb(o, s, [sim.sizes[d] for d in sdims])


def squeeze_field(sim):
    """Drop singleton c/t axes of a sim built by get_sim_from_array."""
    from multiview_stitcher_amd import spatial_image_utils as si

    return sim.isel({d: 0 for d in si.get_nonspatial_dims_from_sim(sim)})


def bb_to_dicts(bb, sdims):
    return {k: dict(zip(sdims, np.asarray(v).tolist())) for k, v in bb.items()}


def union_bb(views_bbs, params, spacing):
    """Union output stack of the views (oracle data model), like calc_fusion_stack_properties."""
    ndim = len(spacing)
    lo, hi = [], []
    for vbb, p in zip(views_bbs, params):
        corners = np.array(list(np.ndindex(*([2] * ndim)))) * (vbb["shape"] - 1) * vbb["spacing"] + vbb["origin"]
        w = corners @ p[:ndim, :ndim].T + p[:ndim, ndim]
        lo.append(w.min(0))
        hi.append(w.max(0))
    lo, hi = np.min(lo, 0), np.max(hi, 0)
    shape = np.floor((hi - lo) / spacing + 1e-9).astype(int) + 1
    return fo.bb(lo, spacing, shape)


def reference_noise_floor(debug, fused_f, eps_w=1.2e-7):
    """Bound on the reference's OWN float32 rounding noise per voxel.

    The reference evaluates the cosine ramp as (cos((1-x)pi)+1)/2 in float32
    (weights.py:502-507): cos() near -1 is rounded to 2^-24, so every ramp weight
    carries an absolute error of ~6e-8 regardless of its size.  Where all
    contributing weights are tiny (tile corners facing the mosaic border) that
    noise is amplified by 1/sum(w):  |d out| <= sum_v |I_v - out| * eps_w / sum_v w_v.
    The HIP kernel evaluates the same ramp as sin^2(pi x/2) (no cancellation), so
    it can differ from the reference by up to this floor; the parity tolerance is
    rtol*|want| + this floor."""
    w, views, trim = debug["raw_weights"], debug["views"], debug["trim"]
    if w is None:
        return np.zeros_like(fused_f, dtype=np.float64)
    sl = (slice(None),) + tuple(slice(t, -t) if t > 0 else slice(None) for t in trim)
    w = w[sl].astype(np.float64)
    v = np.nan_to_num(views[sl].astype(np.float64))
    wsum = w.sum(0)
    spread = (np.abs(v - fused_f.astype(np.float64)[None]) * (w > 0)).sum(0)
    return np.where(wsum > 0, spread * eps_w / np.maximum(wsum, 1e-30), 0.0)


def grid_case(ndim, dtype, tiles, tile_shape, overlap, frac_shift, seed=0, spacing=None):
    """Tiles of a generated mosaic (squeezed sims) and their parameters: identity, or with ``frac_shift`` a fractional translation each."""
    from multiview_stitcher_amd import sample_data

    sims, jit, _ = sample_data.generate_tiled_dataset(
        ndim=ndim, tile_shape=tile_shape, tiles=tiles, overlap=overlap, dtype=dtype, seed=seed, spacing=spacing
    )
    sims = [squeeze_field(s) for s in sims]
    rng = np.random.default_rng(seed + 7)
    params = []
    for s in sims:
        p = np.eye(ndim + 1)
        if frac_shift:
            p[:ndim, ndim] = rng.uniform(-2, 2, ndim)
        params.append(p)
    return sims, params


def run_both(sims, params, out_bb, **kw):
    """One chunk through the oracle and through fusion.fuse_np: (got, want, (want_float, reference_noise_floor))."""
    from multiview_stitcher_amd import fusion, spatial_image_utils as si

    sdims = si.get_spatial_dims_from_sim(sims[0])
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    okw = dict(kw)
    fusion_name = okw.pop("fusion", "weighted_average")
    want, want_f, dbg = fo.fuse_np(list(views), params, out_bb, fusion=fusion_name, full_view_bbs=list(bbs),
                                   return_debug=True, **okw)
    floor = reference_noise_floor(dbg, want_f)
    ffunc = {"weighted_average": fusion.weighted_average_fusion, "max": fusion.max_fusion,
             "simple_average": fusion.simple_average_fusion}[fusion_name]
    got = fusion.fuse_np(
        list(sims), params, bb_to_dicts(out_bb, sdims), fusion_func=ffunc,
        full_view_bbs=[bb_to_dicts(b, sdims) for b in bbs],
        interpolation_order=kw.get("interpolation_order", 1),
        trim_overlap_in_pixels=kw.get("trim_overlap_in_pixels", 0),
        blending_widths=kw.get("blending_widths"),
    )
    return got, want, (want_f, floor)


def fused_close_stats(got, want, want_float=None, rtol=1e-4, data_range=None, max_bad_frac=0.0, noise_floor=None,
                      int_boundary_rtol=1e-4):
    """Parity bar of north_star: float32 fused voxels within 1e-4 relative; integer outputs within
    +-1 LSB (truncating cast after float accumulate) and exact where the float value is not within
    1e-4*|value| of an integer boundary.  ``noise_floor`` (reference_noise_floor) widens the bar by the reference's
    own float32 rounding noise; the returned statistics say how often that was needed and how large it got:
    ``voxels``, ``beyond_plain_bar`` (voxels that pass only thanks to the floor), ``max_floor_used`` (the largest
    floor value among them, in output units), ``lsb_flips`` (integer outputs that differ by one count)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype
    stats = {"voxels": int(got.size), "beyond_plain_bar": 0, "max_floor_used": 0.0, "lsb_flips": 0}
    if np.issubdtype(got.dtype, np.integer):
        diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
        assert diff.max() <= 1, f"integer output differs by {diff.max()} LSB"
        flips = diff == 1
        stats["lsb_flips"] = int(flips.sum())
        if want_float is not None and flips.any():
            frac = want_float - np.floor(want_float)
            dist = np.minimum(frac, 1 - frac)
            plain = dist <= int_boundary_rtol * np.maximum(np.abs(want_float), 1.0)
            floor = noise_floor if noise_floor is not None else np.zeros_like(dist)
            near = dist <= int_boundary_rtol * np.maximum(np.abs(want_float), 1.0) + floor
            assert np.all(near[flips]), "1-LSB flips away from an integer boundary"
            needed = flips & ~plain
            stats["beyond_plain_bar"] = int(needed.sum())
            if needed.any():
                stats["max_floor_used"] = float(np.max(np.broadcast_to(floor, dist.shape)[needed]))
        return stats
    rng = float(data_range) if data_range is not None else float(np.nanmax(np.abs(want)) or 1.0)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    plain_tol = rtol * np.maximum(np.abs(want), 1e-3 * rng)
    tol = plain_tol + noise_floor if noise_floor is not None else plain_tol
    bad = err > tol
    assert bad.mean() <= max_bad_frac, (
        f"{bad.sum()} / {bad.size} voxels beyond rtol={rtol}; worst rel err "
        f"{(err / np.maximum(np.abs(want), 1e-30)).max():.3e}, worst abs {err.max():.3e}"
    )
    needed = (err > plain_tol) & ~bad
    stats["beyond_plain_bar"] = int(needed.sum())
    if needed.any() and noise_floor is not None:
        stats["max_floor_used"] = float(np.max(np.broadcast_to(noise_floor, err.shape)[needed]))
    return stats


def assert_fused_close(got, want, want_float=None, rtol=1e-4, data_range=None, max_bad_frac=0.0, noise_floor=None,
                       max_floor_frac=0.01):
    """fused_close_stats + the bound on how often the reference's noise floor may be needed (<= 1 % of the voxels)."""
    stats = fused_close_stats(got, want, want_float, rtol, data_range, max_bad_frac, noise_floor)
    assert stats["beyond_plain_bar"] <= max_floor_frac * stats["voxels"], stats
    return stats


def white_noise(rng, shape, dtype):
    """Independent white noise over the whole range of ``dtype``: uint16 0..65535, uint8 0..255, float32 in [0, 1)."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return rng.random(shape, dtype=np.float32)
    return rng.integers(0, int(np.iinfo(dtype).max) + 1, size=shape, dtype=dtype)


def placed_tiles(dtype, shape, origins, seed=0):
    """Squeezed sims of ``shape`` with their first voxels at the integer ``origins`` (unit spacing), every one filled with white
    noise of its own (``white_noise``): two views that share a voxel differ by a third of the range on average, so a wrong blend
    weight moves the output by whole counts.  The parameters come separately (``shift_params``)."""
    from multiview_stitcher_amd import spatial_image_utils as si

    ndim = len(shape)
    sdims = ["z", "y", "x"][-ndim:]
    rng = np.random.default_rng(seed)
    sims = []
    for origin in origins:
        sim = si.get_sim_from_array(white_noise(rng, tuple(shape), dtype), dims=sdims, scale=dict(zip(sdims, [1.0] * ndim)),
                                    translation=dict(zip(sdims, [float(v) for v in origin])))
        sims.append(squeeze_field(sim))
    return sims


def stair_tiles(dtype, shape, n, step, seed=0):
    """A "stair" of ``n`` tiles (``placed_tiles``): tile ``i`` at origin ``i * step``."""
    return placed_tiles(dtype, shape, [tuple(i * int(s) for s in step) for i in range(n)], seed)


def grid_origins(tiles, shape, overlap):
    """Origins of a regular grid of ``tiles`` tiles of ``shape`` whose neighbours share ``overlap`` voxels."""
    return [tuple(int(i) * (int(n) - int(o)) for i, n, o in zip(idx, shape, overlap)) for idx in np.ndindex(*tiles)]


def shift_params(ndim, shifts=None, n=None):
    """One translation matrix per view: identity (``shifts`` None, ``n`` of them) or a shift by ``shifts[i]``."""
    params = []
    for i in range(len(shifts) if shifts is not None else n):
        p = np.eye(ndim + 1)
        if shifts is not None:
            p[:ndim, ndim] = shifts[i]
        params.append(p)
    return params


# ---- registration: a shifted pair of crops, and mvs_score_candidates against the oracle (tests/test_reg_gpu.py and others) ----
def _pair(shape, shift, seed=0, sigma=1.0, noise=0.0):
    rng = np.random.default_rng(seed)
    pad = 12
    big = ndimage.gaussian_filter(rng.random(tuple(s + 2 * pad for s in shape)), sigma).astype(np.float32)
    a = np.ascontiguousarray(big[tuple(slice(pad, pad + s) for s in shape)])
    b = np.ascontiguousarray(big[tuple(slice(pad + d, pad + d + s) for d, s in zip(shift, shape))])
    if noise:
        b = b + noise * rng.standard_normal(shape).astype(np.float32)
    return a, b


def _pair_fractional(shape, shift, seed=0, sigma=0.8, noise=0.002):
    """Two float32 windows of one field, the second moved by the FRACTIONAL ``shift`` (b[i] = field[i + shift]): a smoothed
    zero-mean texture of unit standard deviation, 12 samples of margin per side, moved as a whole by the Fourier shift theorem in
    float64, then cropped.  Zero mean: the plain correlation is peaked like the phase-normalised one (no DC pedestal), so both
    normalisations leave a margin between the refinement's maximum and its runner-up (tests/refine_cases.py)."""
    import scipy.fft

    rng = np.random.default_rng(seed)
    pad = 12
    big = ndimage.gaussian_filter(rng.standard_normal(tuple(s + 2 * pad for s in shape)), sigma)
    big /= big.std()
    phase = 1
    for axis, d in enumerate(shift):
        f = scipy.fft.fftfreq(big.shape[axis]).reshape([-1 if k == axis else 1 for k in range(big.ndim)])
        phase = phase * np.exp(2j * np.pi * f * d)
    moved = scipy.fft.ifftn(scipy.fft.fftn(big) * phase).real
    window = tuple(slice(pad, pad + s) for s in shape)
    a = np.ascontiguousarray(big[window]).astype(np.float32)
    b = np.ascontiguousarray(moved[window]).astype(np.float32)
    if noise:
        b = b + noise * rng.standard_normal(shape).astype(np.float32)
    return a, b


def _sparse_pair(shape, shift, seed, invert, blob_frac=0.25, noise=0.0):
    """Zero background with one textured blob; the moving crop holds the same blob displaced by ``shift`` (optionally with
    inverted contrast, which makes the aligned candidate score BELOW an all-background one)."""
    rng = np.random.default_rng(seed)
    a = np.zeros(shape, np.float32)
    b = np.zeros(shape, np.float32)
    ext = [max(8, int(n * blob_frac)) for n in shape]
    lo = [int(n * 0.1) + 6 for n in shape]
    blob = ndimage.gaussian_filter(rng.random(tuple(ext)), 1.0).astype(np.float32) + 0.5
    a[tuple(slice(l, l + e) for l, e in zip(lo, ext))] = blob
    blob_b = (blob.max() + 0.5 - blob) if invert else blob
    if noise:
        blob_b = blob_b + noise * rng.standard_normal(blob.shape).astype(np.float32)
    b[tuple(slice(l - d, l - d + e) for l, d, e in zip(lo, shift, ext))] = np.maximum(blob_b, 0.05)
    return a, b


def _check_scores(a, b, t_cands, region_mode):
    """mvs_score_candidates against the oracle's candidate loop on rescaled inputs."""
    from multiview_stitcher_amd import _reg_ops

    im0, im1 = ro.rescale_intensity_01(a), ro.rescale_intensity_01(b)
    im0nm = np.isnan(im0)
    data_range = np.nanmax([im0, im1]) - np.nanmin([im0, im1])
    im1_min = np.nanmin(im1)
    valid1 = np.sum(~np.isnan(im1))
    im0_bb = ro.get_bb_from_nanmask(~im0nm)
    ssim, spear, codes = _reg_ops.score_candidates(im0, im1, t_cands, region_mode, data_range, im1_min)
    for i, t in enumerate(t_cands):
        code, s, q = ro.score_candidate(im0, im1, im0nm, t, valid1, region_mode, data_range, im1_min, im0_bb)
        assert codes[i] == code, (i, t, codes[i], code)
        if code == 0:
            assert abs(ssim[i] - s) <= 2e-5 * max(abs(s), 1e-3), (i, t, ssim[i], s)
            assert abs(spear[i] - q) <= 1e-5, (i, t, spear[i], q)
        elif code == 1:
            assert ssim[i] == -1 and spear[i] == -1
    # quality_for_all=False: same SSIM / codes; Spearman only for the best-SSIM candidate(s), NaN for the rest
    ssim2, spear2, codes2 = _reg_ops.score_candidates(im0, im1, t_cands, region_mode, data_range, im1_min, quality_for_all=False)
    np.testing.assert_array_equal(codes2, codes)
    np.testing.assert_array_equal(ssim2, ssim)
    listed = [i for i in range(len(codes)) if codes[i] != 2]
    if listed:
        best = np.nanmax([ssim[i] for i in listed])
        for i in listed:
            if ssim[i] == best or codes[i] == 1:
                assert spear2[i] == spear[i], (i, spear2[i], spear[i])
            else:
                assert np.isnan(spear2[i])


# ---- what the apply tests of test_intensity_gpu.py and test_shading_gpu.py share ----
def apply_input(shape, dtype, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        x = (rng.random(shape) * 200 - 50).astype(np.float32)
        x.ravel()[::7] = np.nan
        return x
    hi = np.iinfo(dtype).max
    x = rng.integers(0, hi + 1, size=shape).astype(dtype)
    x.ravel()[::5] = hi
    x.ravel()[1::5] = 0
    return x


def apply_coeff(cells, dtype, seed):
    """Gains 0.4 .. 1.9 and offsets on both sides of zero, large enough to saturate integer outputs at both ends; ``cells``: the
    shape of the coefficient grid (cells per axis, or the pixels of a plane)."""
    rng = np.random.default_rng(seed)
    span = 1.0 if dtype == np.float32 else float(np.iinfo(dtype).max)
    return np.stack([rng.random(cells) * 1.5 + 0.4, (rng.random(cells) - 0.5) * 0.8 * span], axis=-1).astype(np.float32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
