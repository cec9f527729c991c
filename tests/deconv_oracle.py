"""numpy / scipy restatement of the reference's multi-view deconvolution (fusion/mv_deconv.py), used by the tests as a
checker only.  Every step cites the reference line it restates; the project's implementation (multiview_stitcher_amd
.mv_deconv + csrc/mvs_deconv.hip) is never called from here."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

PSF_TYPES = ("EFFICIENT_BAYESIAN", "OPTIMIZATION_I", "OPTIMIZATION_II", "INDEPENDENT")   # mv_deconv.py:24-54


def norm(kernel):
    """mv_deconv.py:85-91: sum to 1 in float64, returned as float32."""
    k = np.asarray(kernel, dtype=np.float64)
    s = k.sum()
    if s > 0:
        k = k / s
    return k.astype(np.float32)


def gaussian_psf(sigma, ndim=None, shape=None):
    """mv_deconv.py:98-129: a delta at the centre of ceil(6 sigma) | 1, filtered by gaussian_filter, normalised."""
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    if sigma.size == 1 and ndim is not None:
        sigma = np.full(ndim, float(sigma[0]))
    if shape is None:
        shape = tuple(int(np.ceil(6.0 * s)) | 1 for s in sigma)
    delta = np.zeros(shape, np.float32)
    delta[tuple(n // 2 for n in shape)] = 1.0
    return norm(ndimage.gaussian_filter(delta, sigma=sigma.tolist()))


def psf_from_spacing(spacing, na=0.8, wavelength_um=0.5):
    """mv_deconv.py:132-167: sigma_lateral = 0.5 lambda / NA, sigma_axial = 2 lambda / NA^2, in pixels, at least 0.5."""
    lateral, axial = 0.5 * wavelength_um / na, 2.0 * wavelength_um / na ** 2
    return gaussian_psf([max(0.5, (axial if d == "z" else lateral) / float(s)) for d, s in spacing.items()])


def _conv0(a, b):
    return ndimage.convolve(a, b, mode="constant", cval=0.0)


def back_kernel(v, psfs, psf_type):
    """mv_deconv.py:172-247: the compound back-projection kernel of view v (float64 products, normalised to float32)."""
    psf_type = getattr(psf_type, "value", psf_type)
    p = np.asarray(psfs[v], np.float64)
    pf = np.flip(p)
    if len(psfs) == 1 or psf_type == "INDEPENDENT":
        return norm(pf)
    if psf_type == "OPTIMIZATION_II":
        return norm(np.flip(p ** len(psfs)))
    acc = p.copy() if psf_type == "OPTIMIZATION_I" else pf.copy()
    for w, q in enumerate(psfs):
        if w == v:
            continue
        q = np.asarray(q, np.float64)
        c = _conv0(pf, q)
        if psf_type != "OPTIMIZATION_I":
            c = _conv0(c, np.flip(q))
        acc = acc * c
    return norm(np.flip(acc)) if psf_type == "OPTIMIZATION_I" else norm(acc)


def kernels(n_views, ndim, psfs=None, psf_type="EFFICIENT_BAYESIAN", output_spacing=None, na=0.8, wavelength_um=0.5):
    """mv_deconv.py:363-404: the forward PSFs (padded to one shape, (d//2, d - d//2)) and the back-projection kernels."""
    if psfs is None:
        p0 = psf_from_spacing(output_spacing, na, wavelength_um) if output_spacing is not None else gaussian_psf(1.5, ndim=ndim)
        ks = [p0] * n_views
    else:
        if len(psfs) != n_views:
            raise ValueError(f"len(psfs) = {len(psfs)}, but n_views = {n_views}")
        ks = [norm(np.asarray(p).astype(np.float32)) for p in psfs]
    big = tuple(max(k.shape[d] for k in ks) for d in range(ndim))
    out = []
    for k in ks:
        if k.shape != big:
            k = np.pad(k, [((t - a) // 2, (t - a) - (t - a) // 2) for a, t in zip(k.shape, big)])
        out.append(norm(k))
    return out, [back_kernel(v, out, psf_type) for v in range(n_views)]


def forward_convolve(psi, kernel):
    """mv_deconv.py:437-440: the forward projection."""
    return ndimage.convolve(psi, kernel, mode="mirror")


def back_convolve(wr, kernel):
    """mv_deconv.py:464-467: the back projection."""
    return ndimage.convolve(wr, kernel, mode="constant", cval=1.0)


def deconvolve(views, blend, psfs=None, psf_type="EFFICIENT_BAYESIAN", n_iterations=10, lambda_reg=0.0, min_value=1e-4,
               output_spacing=None, na=0.8, wavelength_um=0.5, sample_boundary_erosion_px=0, convolutions=None):
    """mv_deconv.py:251-501 on host arrays.  ``convolutions``: an optional (forward, back) pair of callables
    f(array, kernel) -> array replacing forward_convolve / back_convolve (the tests inject deliberate mistakes with it)."""
    fwd, back = convolutions or (forward_convolve, back_convolve)
    views = np.asarray(views)
    n_views, ndim, dtype = views.shape[0], views.ndim - 1, views.dtype
    covered = ~np.isnan(views)                                                     # :354-355
    obs = np.nan_to_num(views, nan=0.0)
    k1, k2 = kernels(n_views, ndim, psfs, psf_type, output_spacing, na, wavelength_um)
    mv = np.float32(min_value)
    psi = np.nansum(obs * blend, axis=0).astype(np.float32).clip(mv)                # :409-410
    peak = float(psi.max())                                                          # :412-414
    if peak <= 0:
        peak = 1.0
    one = np.float32(1.0)
    for _ in range(n_iterations):                                                    # :428-483
        for v in range(n_views):
            blurred = fwd(psi, k1[v])
            ratio = np.where(covered[v], obs[v] / np.maximum(blurred, mv), np.ones_like(blurred))
            wr = one + blend[v] * (ratio - one)
            value = psi * back(wr, k2[v])
            if lambda_reg > 0:
                x = np.maximum(value, np.float32(0.0)) / peak
                value = (np.sqrt(one + np.float32(2.0 * lambda_reg) * x) - one) / np.float32(lambda_reg) * peak
            psi = np.where(np.isnan(value), mv, np.maximum(value, mv))
    if sample_boundary_erosion_px > 0:                                               # :485-499
        keep = ndimage.binary_erosion(np.any(covered, axis=0), iterations=sample_boundary_erosion_px, border_value=1,
                                      brute_force=True)
        psi = np.where(keep, psi, np.float32(0.0))
    return psi.astype(dtype)


def required_overlap(kwargs):
    """mv_deconv.py:504-527."""
    kwargs = kwargs or {}
    if kwargs.get("output_spacing") is not None:
        size = max(psf_from_spacing(kwargs["output_spacing"], kwargs.get("na", 0.8), kwargs.get("wavelength_um", 0.5)).shape)
    else:
        size = int(np.ceil(6.0 * 1.5)) | 1
    return size // 2


# --- seeded cases of tests/golden/mv_deconv_ref.npz (inputs are regenerated from the seeds; the fixture stores outputs) ---
def _views(seed, n_views, shape, nan_views=()):
    """Smooth positive views (background >= 10) and normalised blending weights; views listed in ``nan_views`` lose a
    slab (NaN = outside the view) that their weight then excludes."""
    rng = np.random.default_rng(seed)
    base = ndimage.gaussian_filter(rng.random(shape), 1.0) * 200.0 + 10.0
    views = np.stack([base * (0.8 + 0.4 * rng.random()) + rng.random(shape) * 5.0 for _ in range(n_views)]).astype(np.float32)
    w = rng.random((n_views,) + tuple(shape)).astype(np.float32) + np.float32(0.05)
    for v in nan_views:
        views[v][..., : max(1, shape[-1] // 3)] = np.nan
    w = w * ~np.isnan(views)
    s = np.nansum(w, axis=0)
    s[s == 0] = 1
    return views, (w / s).astype(np.float32)


def _psf2(seed, shape):
    return np.random.default_rng(seed).random(shape).astype(np.float32) + np.float32(0.1)


def cases():
    """name -> (views, blending_weights, kwargs of multi_view_deconvolution)."""
    out = {}
    v, w = _views(1, 2, (16, 20, 24), nan_views=(1,))
    out["3d_default"] = (v, w, {})
    for i, t in enumerate(PSF_TYPES):
        v, w = _views(10 + i, 3, (36, 44), nan_views=(0,))
        out[f"2d_{t}"] = (v, w, dict(psf_type=t, psfs=[gaussian_psf([1.0, 1.5]), gaussian_psf([2.0, 1.0]), gaussian_psf(1.2, ndim=2)]))
    v, w = _views(20, 2, (12, 18, 20))
    out["3d_OPTIMIZATION_I_spacing"] = (v, w, dict(psf_type="OPTIMIZATION_I", output_spacing={"z": 2.0, "y": 0.5, "x": 0.5}))
    v, w = _views(21, 2, (30, 34), nan_views=(1,))
    out["2d_nonseparable"] = (v, w, dict(psfs=[_psf2(5, (5, 7)), gaussian_psf(1.0, ndim=2)]))
    v, w = _views(22, 2, (30, 34))
    out["2d_even"] = (v, w, dict(psfs=[_psf2(6, (4, 6)), _psf2(7, (4, 6))], psf_type="INDEPENDENT"))
    v, w = _views(23, 2, (14, 18, 20), nan_views=(0,))
    out["3d_lambda_erosion"] = (v, w, dict(lambda_reg=0.01, sample_boundary_erosion_px=2))
    v, w = _views(24, 2, (3, 20, 22), nan_views=(1,))
    out["3d_thin"] = (v, w, {})
    v, w = _views(25, 2, (3, 40))
    out["2d_thin"] = (v, w, dict(psf_type="OPTIMIZATION_II"))
    v, w = _views(26, 1, (24, 28))
    out["2d_one_view"] = (v, w, dict(min_value=1e-3))
    v, w = _views(27, 2, (10, 14, 18), nan_views=(0,))
    out["3d_even_asymmetric"] = (v, w, dict(psfs=[_psf2(8, (4, 6, 4)), _psf2(9, (4, 6, 4))]))
    v, w = _views(28, 2, (10, 14, 18))
    out["3d_rank1_asymmetric"] = (v, w, dict(psfs=[_rank1(10, (3, 4, 5)), _rank1(11, (3, 4, 5))], psf_type="OPTIMIZATION_I"))
    return out


# --- edge cases of the GPU kernels (tile edges, wide / even / asymmetric kernels, thin chunks, zero coverage); checked
# against deconvolve() directly, never stored in the fixture ---
def _hf_views(seed, n_views, shape, holes=False):
    """Views with high-frequency content (white noise plus sparse bright beads, so a shifted or flipped kernel shows)
    and normalised blending weights.  ``holes``: every view loses a border block and an interior block (NaN), so some
    voxels have no view at all and their weights normalise 0 -> 0 / 1."""
    rng = np.random.default_rng(seed)
    base = rng.random(shape) * 100.0 + 20.0
    base[rng.random(shape) < 0.01] += 1500.0
    views = np.stack([base * (0.8 + 0.4 * rng.random()) + rng.random(shape) * 20.0 for _ in range(n_views)]).astype(np.float32)
    if holes:
        corner = tuple(slice(0, max(1, n // 3)) for n in shape)
        inner = tuple(slice(n // 2, n // 2 + max(1, n // 5)) for n in shape)
        views[(slice(None),) + corner] = np.nan
        views[(slice(None),) + inner] = np.nan
    w = rng.random((n_views,) + tuple(shape)).astype(np.float32) + np.float32(0.05)
    w = w * ~np.isnan(views)
    s = np.nansum(w, axis=0)
    s[s == 0] = 1
    return views, (w / s).astype(np.float32)


def _rand_psf(seed, shape):
    """A random positive PSF that is far from rank 1 and from symmetric (a few taps dominate)."""
    return (np.random.default_rng(seed).random(shape) ** 6 + 0.01).astype(np.float32)


def _rank1(seed, shape):
    """Outer product of random asymmetric positive 1-D factors: rank 1, so it takes the separable path."""
    rng = np.random.default_rng(seed)
    k = np.ones((), np.float64)
    for n in shape:
        k = np.multiply.outer(k, rng.random(n) ** 2 + 0.05)
    return k.astype(np.float32)


def edge_cases():
    """name -> (views, blending_weights, kwargs of multi_view_deconvolution, n_iterations)."""
    out = {}
    # 2D: partial x and y tiles of the direct path (64 x 32), the widest window (kx = 63 -> kxp = 64), an even PSF padded
    # asymmetrically to the common shape, a halo taller than the tile (ky = 63), kx = 5 -> kxp = 8
    v, w = _hf_views(100, 2, (100, 200))
    out["2d_wide_63x63"] = (v, w, dict(psfs=[_rand_psf(101, (63, 63)), _rand_psf(102, (61, 62))]), 1)
    v, w = _hf_views(103, 2, (90, 150))
    out["2d_tall_63x5"] = (v, w, dict(psfs=[_rand_psf(104, (63, 5)), _rand_psf(105, (63, 5))]), 1)
    v, w = _hf_views(106, 2, (40, 140))
    out["2d_flat_5x63"] = (v, w, dict(psfs=[_rand_psf(107, (5, 63)), _rand_psf(108, (4, 62))], psf_type="INDEPENDENT"), 2)
    v, w = _hf_views(109, 2, (70, 130))
    out["2d_even_62x4"] = (v, w, dict(psfs=[_rand_psf(110, (62, 4)), _rand_psf(111, (62, 4))], psf_type="OPTIMIZATION_II"), 2)
    # 3D direct path across x and y tiles, flip and origin along every axis
    v, w = _hf_views(112, 2, (7, 45, 150))
    out["3d_direct_odd"] = (v, w, dict(psfs=[_rand_psf(113, (5, 7, 9)), _rand_psf(114, (5, 7, 9))]), 2)
    v, w = _hf_views(115, 2, (7, 45, 150))
    out["3d_direct_even"] = (v, w, dict(psfs=[_rand_psf(116, (4, 6, 8)), _rand_psf(117, (4, 6, 8))]), 2)
    # 3D separable path: asymmetric and even factors, every compound kernel type
    for i, t in enumerate(PSF_TYPES):
        for parity, ks in (("even", (4, 6, 10)), ("odd", (5, 7, 9))):
            v, w = _hf_views(120 + 2 * i + (parity == "odd"), 2, (9, 40, 130))
            psfs = [_rank1(130 + 4 * i + 2 * (parity == "odd"), ks), _rank1(131 + 4 * i + 2 * (parity == "odd"), ks)]
            out[f"3d_rank1_{parity}_{t}"] = (v, w, dict(psfs=psfs, psf_type=t), 2)
    # a length-1 kernel axis; kx a multiple of 4 (no x padding)
    v, w = _hf_views(150, 2, (8, 30, 140))
    out["3d_ky1_kx12"] = (v, w, dict(psfs=[_rand_psf(151, (5, 1, 12)), _rand_psf(152, (5, 1, 12))]), 2)
    v, w = _hf_views(153, 2, (8, 30, 140))
    out["3d_rank1_kz1_kx12"] = (v, w, dict(psfs=[_rank1(154, (1, 7, 12)), _rank1(155, (1, 7, 12))]), 2)
    # chunks thinner than the kernel: mirror wraps periodically, a length-1 axis is constant (rank 1: both paths)
    v, w = _hf_views(156, 2, (1, 40, 70))
    out["3d_nz1_kz9"] = (v, w, dict(psfs=[_rank1(157, (9, 5, 6)), _rank1(158, (9, 5, 6))]), 2)
    v, w = _hf_views(159, 2, (2, 30, 70))
    out["3d_nz2_kz15"] = (v, w, dict(psfs=[_rank1(160, (15, 3, 5)), _rank1(161, (15, 3, 5))]), 2)
    v, w = _hf_views(162, 2, (10, 3, 70))
    out["3d_ny3_ky15"] = (v, w, dict(psfs=[_rank1(163, (3, 15, 5)), _rank1(164, (3, 15, 5))]), 2)
    # voxels no view covers (a border block and an interior hole in every view), 2D erosion, the peak of lambda_reg
    for ndim, shape in ((2, (40, 60)), (3, (10, 30, 40))):
        for erosion, lam in ((0, 0.01), (3, 0.0), (3, 0.01)):
            v, w = _hf_views(170 + 10 * ndim + erosion + int(lam > 0), 2, shape, holes=True)
            kw = dict(sample_boundary_erosion_px=erosion, lambda_reg=lam)
            out[f"{ndim}d_uncovered_erosion{erosion}_lambda{int(lam > 0)}"] = (v, w, kw, 2)
    # the view count of the separable path's per-view tables
    for n in (64, 65):
        v, w = _hf_views(200 + n, n, (16, 20))
        out[f"2d_views{n}"] = (v, w, {}, 1)
    # no iteration: init, clamp, erosion mask and cast only
    v, w = _hf_views(210, 2, (6, 20, 30), holes=True)
    out["3d_zero_iterations"] = (v, w, dict(sample_boundary_erosion_px=1), 0)
    return out


# mistakes each edge case must catch (tests/test_mv_deconv_host.py injects them through deconvolve's ``convolutions``):
# flip_<axis> flips the kernel along one axis, origin_<axis> shifts it by one voxel along an even axis, reflect uses
# mode "reflect" for the forward projection, cval0 pads the back projection with 0, sep_cval1 runs the back projection
# as three 1-D passes whose later passes pad with 1 instead of the product of the earlier factors' sums.
def edge_mutations():
    flips2, flips3 = ("flip_y", "flip_x"), ("flip_z", "flip_y", "flip_x")
    bounds = ("reflect", "cval0")
    out = {
        "2d_wide_63x63": flips2 + bounds,
        "2d_tall_63x5": flips2 + bounds,
        "2d_flat_5x63": flips2 + bounds,
        "2d_even_62x4": flips2 + ("origin_y", "origin_x") + bounds,
        "3d_direct_odd": flips3 + bounds,
        "3d_direct_even": flips3 + ("origin_z", "origin_y", "origin_x") + bounds,
        "3d_ky1_kx12": ("flip_z", "flip_x", "origin_x") + bounds,
        "3d_rank1_kz1_kx12": ("flip_y", "flip_x", "origin_x") + bounds + ("sep_cval1",),
        "3d_nz1_kz9": flips2 + bounds + ("sep_cval1",),
        "3d_nz2_kz15": flips2 + bounds + ("sep_cval1",),
        "3d_ny3_ky15": ("flip_z", "flip_x") + bounds + ("sep_cval1",),
        "2d_views64": bounds,
        "2d_views65": bounds,
    }
    for t in PSF_TYPES:
        out[f"3d_rank1_even_{t}"] = flips3 + ("origin_z", "origin_y", "origin_x") + bounds + ("sep_cval1",)
        out[f"3d_rank1_odd_{t}"] = flips3 + bounds + ("sep_cval1",)
    for ndim in (2, 3):
        for erosion, lam in ((0, 1), (3, 0), (3, 1)):
            out[f"{ndim}d_uncovered_erosion{erosion}_lambda{lam}"] = bounds
    return out


FIXTURE_ITERATIONS = 3


def helper_cases():
    """name -> (function name, args) of the PSF helpers the fixture stores."""
    return {
        "gauss_iso3": ("make_gaussian_psf", (1.5,), {"ndim": 3}),
        "gauss_aniso2": ("make_gaussian_psf", ([1.0, 2.2],), {}),
        "gauss_shape": ("make_gaussian_psf", ([0.8, 1.3],), {"shape": (5, 6)}),
        "est_iso": ("estimate_psf", ({"z": 1.0, "y": 1.0, "x": 1.0},), {}),
        "est_aniso": ("estimate_psf", ({"z": 2.5, "y": 0.2, "x": 0.25},), {"na": 1.1, "wavelength_um": 0.6}),
        "est_2d": ("estimate_psf", ({"y": 0.3, "x": 0.3},), {}),
    }


def compound_inputs():
    """Three 3-D PSFs of one shape for the compound-kernel entries of the fixture."""
    return [gaussian_psf([1.0, 1.2, 0.9], shape=(7, 7, 7)), gaussian_psf([1.6, 0.8, 1.0], shape=(7, 7, 7)),
            gaussian_psf(1.1, ndim=3, shape=(7, 7, 7))]
