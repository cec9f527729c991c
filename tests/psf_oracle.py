"""numpy / scipy restatement of the PSF extraction from beads (mv_deconv.extract_psf, csrc/mvs_psf.hip), used by the tests as a
checker only: float64 throughout, samples by scipy.ndimage.map_coordinates(order=1, mode="constant", cval=nan) on float64 data,
the steps in the order the contract lists them.  The project's implementation is never called from here."""
from __future__ import annotations

import numpy as np
from scipy import ndimage

STATUS = ("used", "outside", "empty")


def window_matrix(spacing, affine, output_spacing):
    """Step 1: M = diag(1 / spacing) L^-1 diag(output_spacing), L the linear part of the view -> world affine."""
    spacing = np.asarray(spacing, dtype=np.float64)
    ndim = len(spacing)
    lin = np.asarray(affine, dtype=np.float64)[:ndim, :ndim]
    return np.linalg.inv(lin) / spacing[:, None] * np.asarray(output_spacing, dtype=np.float64)[None, :]


def offsets(radius):
    """All window offsets, (n, ndim) integers with the last axis fastest, and the mask of the shell among them."""
    grids = np.meshgrid(*[np.arange(-r, r + 1) for r in radius], indexing="ij")
    o = np.stack([g.reshape(-1) for g in grids], axis=1)
    return o, np.any(np.abs(o) == np.asarray(radius)[None, :], axis=1)


def too_close(centers, matrix, radius, chunk=256):
    """Step 2: beads a != b with |(M^-1 (c_b - c_a))_k| < 2 r_k + 1 on every axis are both marked (chunked, no n x n doubles)."""
    q = np.linalg.solve(matrix, np.asarray(centers, dtype=np.float64).T).T
    lim = 2.0 * np.asarray(radius, dtype=np.float64) + 1.0
    mask = np.zeros(len(q), dtype=bool)
    for a0 in range(0, len(q), chunk):
        near = np.all(np.abs(q[a0:a0 + chunk, None, :] - q[None, :, :]) < lim, axis=2)
        near[np.arange(near.shape[0]), a0 + np.arange(near.shape[0])] = False
        mask[a0:a0 + chunk] |= near.any(axis=1)
    return mask


def sample_window(view64, center, matrix, o):
    """Step 3: the view at c + M o; NaN = out of bounds."""
    coords = center[:, None] + matrix @ o.T.astype(np.float64)
    return ndimage.map_coordinates(view64, coords, order=1, mode="constant", cval=np.nan)


def extract(view, centers, matrix, radius, refine_iterations=1):
    """Steps 3-7 for beads at the pixel coordinates ``centers``.  Returns a dict: ``psf`` (float64, shape 2 r + 1; zeros when no
    bead is used), ``centers`` (where each bead was last sampled), ``status`` (strings), ``background``, ``energy``, ``ncc``
    (NaN where a bead did not get that far), ``windows`` (the u_b of the used beads, by bead index)."""
    view64 = np.asarray(view, dtype=np.float64)
    centers = np.array(centers, dtype=np.float64, copy=True)
    matrix = np.asarray(matrix, dtype=np.float64)
    o, shell = offsets(radius)
    n = len(centers)
    status = ["used"] * n
    background, energy, ncc = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    windows = {}
    for b in range(n):
        for it in range(refine_iterations + 1):
            s = sample_window(view64, centers[b], matrix, o).astype(np.float32).astype(np.float64)      # (a sample is a float32)
            if np.isnan(s).any():
                status[b] = "outside"
                break
            bg = s[shell].mean()
            e = np.maximum(s - bg, 0.0)
            background[b], energy[b] = bg, e.sum()
            if not e.sum() > 0:
                status[b] = "empty"
                break
            if it == refine_iterations:
                windows[b] = e / e.sum()
                break
            centers[b] = centers[b] + matrix @ ((o * e[:, None]).sum(axis=0) / e.sum())
        if status[b] == "outside":
            background[b] = energy[b] = np.nan
    shape = tuple(2 * r + 1 for r in radius)
    acc = np.zeros(len(o))
    for b in sorted(windows):
        acc = acc + windows[b]
    psf = acc / len(windows) if windows else acc
    for b, u in windows.items():
        du, dp = u - u.mean(), psf - psf.mean()
        ncc[b] = (du * dp).sum() / np.sqrt((du * du).sum() * (dp * dp).sum())
    return {"psf": psf.reshape(shape), "centers": centers, "status": status, "background": background, "energy": energy, "ncc": ncc,
            "windows": {b: u.reshape(shape) for b, u in windows.items()}}


def extract_psf(view, spacing, origin, points, psf_shape, affine=None, output_spacing=None, refine_iterations=1, min_correlation=None,
                max_beads=None):
    """The whole of mv_deconv.extract_psf(..., return_info=True) on plain arrays: (float32 PSF of unit sum, info)."""
    ndim = view.ndim
    spacing, origin = np.asarray(spacing, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    radius = [(int(n) - 1) // 2 for n in psf_shape]
    matrix = window_matrix(spacing, np.eye(ndim + 1) if affine is None else affine, spacing if output_spacing is None else output_spacing)
    points = np.asarray(points, dtype=np.float64)
    centers = (points - origin) / spacing
    status = np.array(["used"] * len(points), dtype=object)
    status[too_close(centers, matrix, radius)] = "too_close"
    sel = np.nonzero(status == "used")[0]
    if max_beads is not None:
        status[sel[max_beads:]] = "skipped"
        sel = sel[:max_beads]
    res = extract(view, centers[sel], matrix, radius, refine_iterations)
    centers[sel] = res["centers"]
    status[sel] = res["status"]
    background, ncc = np.full(len(points), np.nan), np.full(len(points), np.nan)
    background[sel], ncc[sel] = res["background"], res["ncc"]
    used = sel[np.asarray(res["status"]) == "used"]
    psf = res["psf"]
    if min_correlation is not None and len(used):
        low = used[~(ncc[used] >= min_correlation)]
        if len(low):
            status[low] = "low_correlation"
            used = used[ncc[used] >= min_correlation]
            if len(used):
                res = extract(view, centers[used], matrix, radius, 0)
                status[used] = res["status"]
                background[used], ncc[used] = res["background"], res["ncc"]
                psf = res["psf"]
                used = used[np.asarray(res["status"]) == "used"]
    if len(used) == 0:
        raise ValueError("no usable bead")
    total = psf.sum()
    return (psf / total).astype(np.float32), {"centers": origin + centers * spacing, "status": [str(v) for v in status],
                                              "background": background, "ncc": ncc, "n_used": int(len(used))}


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
def gaussian_beads(shape, positions, amplitudes, sigma, background):
    """background + sum_b amplitude_b exp(-sum_k (x_k - p_bk)^2 / (2 sigma_k^2)), float64."""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    out = np.full(shape, float(background))
    for p, a in zip(positions, amplitudes):
        out += a * np.exp(-sum((g - pk) ** 2 / (2.0 * s * s) for g, pk, s in zip(grids, p, sigma)))
    return out


FIXTURE_A_SHAPE = (40, 48, 56)
FIXTURE_A_RADIUS = (6, 4, 5)
FIXTURE_A_DOUBLET = 4
FIXTURE_A_MIN_CORRELATION = 0.97


def fixture_a(dtype=np.float32):
    """(view, true positions (18, 3), positions handed in = the true ones rounded).  18 Gaussian beads of sigma (2.0, 1.2, 1.5) on
    a 2 x 3 x 3 lattice, jittered by up to half a pixel, over a background of 100; bead 4 has a twin of its own amplitude 2.5 px
    further along y that is in no point list.  uint16: the same data rounded; uint8: amplitudes scaled to <= 200, background 20."""
    rng = np.random.default_rng(3)
    lattice = np.array([(z, y, x) for z in (9, 29) for y in (8, 22, 38) for x in (9, 27, 45)], dtype=np.float64)
    truth = lattice + rng.uniform(-0.5, 0.5, lattice.shape)
    amp = rng.uniform(500.0, 3000.0, len(lattice))
    background = 100.0
    if np.dtype(dtype) == np.uint8:
        amp, background = amp * (200.0 / 3000.0), 20.0
    twin = truth[FIXTURE_A_DOUBLET] + np.array([0.0, 2.5, 0.0])
    view = gaussian_beads(FIXTURE_A_SHAPE, list(truth) + [twin], list(amp) + [amp[FIXTURE_A_DOUBLET]], (2.0, 1.2, 1.5), background)
    if np.dtype(dtype) != np.float32:
        view = np.rint(view)
    return np.ascontiguousarray(view.astype(dtype)), truth, np.rint(truth)
