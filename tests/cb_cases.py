"""Case table of the content-based fusion tests (tests/test_cb_cases_host.py, tests/test_fuse_content_based_gpu.py): chunks that the
default content-based path (csrc/mvs_gauss_fast.inc) declines, so that the bit-faithful passes of csrc/mvs_gauss.hip run without any
option set.  A case is ``(sims, params, out_bb, sigmas, kwargs)``: squeezed sims, one view -> world matrix per view, the chunk's box in
the oracle's data model, (sigma_1, sigma_2), and the trim.  The host test proves with the oracle alone that every case is what it says
it is; the GPU test runs the library on it.

Turned, sheared and mirrored views (``tests/affine_cases.py``, sigmas (1.0, 2.0): radii 4 and 8) -- declined for kCbMatrix:

  fan2d_12, fan3d_12   12 views (more than 8: boxes in global memory, the kernels that are not "small"), every one turned
  shear_aniso          3 views, boxes that start inside the chunk; the third view reaches the chunk with a corner only
  trimmed              shear_aniso under trim 3
  far_origin           offsets near 1e5
  mirror_swap          exact permutation and sign matrices; float32 tiles hold NaNs
  mirror_swap_one_rotated   three identity pixel matrices and one turned view
  lightsheet_pair      two 3D views of spacing (2, 1, 1), the second turned by 90 + 3 degrees about y and moved by a fraction of a
                       voxel; sigmas (1.5, 3.0)

Translation grids (``helpers.grid_case``, fractional shifts):

  short_z3, short_z7, short_z_default, one_plane, short_y_2d, stray_views     kCbShortAxis: a chunk axis shorter than a radius
  radius_128           kCbRadius: sigma_2 = 32
  long_y, mid_y        kCbLine: y lines no tile of the default path holds
  nine_views_3d        kCbViewCount

A chunk with a short axis comes from ``fuse_np`` (or ``mvs_fuse_chunk``) called directly: ``fuse()`` adds the halo 2 * sigma_2 on both
sides of every axis of a chunk, so its chunks are at least 4 * sigma_2 long -- the radius int(4 * sigma_2 + 0.5) at least.

``plan`` restates the integer rules of csrc/mvs_cb_plan.h (which path, which line kernels); tests/native/cb_plan_host_test.cpp checks
the header itself."""
import functools

import numpy as np

from oracle import fuse_oracle as fo
from tests import affine_cases as ac
from tests.helpers import grid_case, reference_noise_floor, sim_to_view, union_bb, white_noise

U16, U8, F32 = np.dtype(np.uint16), np.dtype(np.uint8), np.dtype(np.float32)
ROTATED = ("fan2d_12", "fan3d_12", "shear_aniso", "trimmed", "far_origin", "mirror_swap", "mirror_swap_one_rotated", "lightsheet_pair")
SHORT_AXIS = ("short_z3", "short_z7", "one_plane", "short_z_default", "short_y_2d", "stray_views")
GRIDS = SHORT_AXIS + ("radius_128", "long_y", "mid_y", "nine_views_3d")
NAMES = ROTATED + GRIDS
# the one decline reason (CbDecline of csrc/mvs_cb_plan.h) a case is in the table for
REASON = dict({n: "kCbMatrix" for n in ROTATED}, **{n: "kCbShortAxis" for n in SHORT_AXIS},
              radius_128="kCbRadius", long_y="kCbLine", mid_y="kCbLine", nine_views_3d="kCbViewCount")
# views that take no part (stray_views: the fifth view lies wholly outside the chunk)
ABSENT = {"stray_views": (4,)}
STRAY_OUTSIDE, STRAY_ROW = 4, 5


def cells():
    """(name, dtype, order) of every GPU cell."""
    out = [("fan2d_12", d, o) for d in (U16, U8, F32) for o in (0, 1)]
    out += [(n, d, 1) for n in ("fan3d_12", "shear_aniso") for d in (U16, F32)]
    out += [("trimmed", d, o) for d in (U16, F32) for o in (0, 1)]
    out += [("far_origin", F32, 1)]
    out += [("mirror_swap", d, o) for d in (U8, F32) for o in (0, 1)]
    out += [("mirror_swap_one_rotated", U16, 1)]
    out += [("lightsheet_pair", d, 1) for d in (U16, F32)]
    out += [(n, d, 1) for n in GRIDS for d in (U16, F32)]
    return out


def cell_id(cell):
    name, dtype, order = cell
    return f"{name}-{np.dtype(dtype).name}-order{order}"


LIGHTSHEET_SPACING = np.array([2.0, 1.0, 1.0])


def _lightsheet_pair(dtype):
    """Two stacks of 22 planes, 2.0 apart, of 40 x 44 pixels: the second one acquired after turning the sample by 90 degrees about y
    (its planes lie along the first one's x), 3 degrees more than that, and off by a fraction of a voxel."""
    rng = np.random.default_rng(61)
    shape = (22, 40, 44)
    sims = [ac._tile(white_noise(rng, shape, dtype), LIGHTSHEET_SPACING, np.zeros(3)) for _ in range(2)]
    c = ac._centre(shape, LIGHTSHEET_SPACING, np.zeros(3))
    a = np.deg2rad(93.0)
    about_y = np.array([[np.cos(a), 0.0, -np.sin(a)], [0.0, 1.0, 0.0], [np.sin(a), 0.0, np.cos(a)]])
    params = [np.eye(4), ac._about(about_y, c, [0.37, -0.61, 0.23])]
    return sims, params, fo.bb([-0.5, -0.25, -0.5], np.ones(3), (44, 40, 44)), (1.5, 3.0), {}


def _grid(ndim, dtype, tiles, tile_shape, overlap, seed, sigmas, trim=0):
    sims, params = grid_case(ndim, dtype, tiles, tile_shape, overlap, True, seed=seed)
    _, bbs = zip(*[sim_to_view(s) for s in sims])
    return sims, params, union_bb(bbs, params, np.ones(ndim)), sigmas, ({"trim_overlap_in_pixels": trim} if trim else {})


# seeds of the grids: from 4 (the short axes), 52 (long_y, mid_y), 53 (radius_128) and 54 (nine_views_3d) on, the first one at which
# tests/test_cb_cases_host.py holds; short_z_default is the only one that had to move (the weight margin: 5.5e-6 at seed 4)
SEEDS = {"short_z3": 4, "short_z7": 4, "one_plane": 4, "short_z_default": 28, "short_y_2d": 4, "stray_views": 4, "radius_128": 53,
         "long_y": 52, "mid_y": 52, "nine_views_3d": 54}


def _one_plane(dtype):
    sims, params, union, sigmas, kw = _grid(3, dtype, (1, 2, 2), (5, 40, 44), (0, 12, 14), SEEDS["one_plane"], (1.5, 3.0))
    origin, shape = union["origin"].copy(), union["shape"].copy()
    origin[0] += 3.0          # a plane that every tile reaches (the shifts lie within +-2)
    shape[0] = 1
    return sims, params, fo.bb(origin, np.ones(3), shape), sigmas, kw


# The corners of a long tile.  The reference interpolates its blending weight from a 5-point table per axis, so between the two outer
# nodes of both axes the ramp argument is the PRODUCT (1 + cy) / (n_y + 1) * (1 + cx) / 10 * 4.1 (cy, cx: coordinates from the corner):
# for n_y = 1600 or 1760 the weight (pi x / 2)^2 is about 1.5e-7 at the corner voxel and stays below 1e-5 while (1 + cy) (1 + cx) < 9,
# whatever the shifts are.  No seed moves that, so these two chunks leave the corners of their tiles out: long_y ends 13 rows inside both
# tiles (their boxes span the chunk along y: reflection at both ends, constant lines of the mask), mid_y is as narrow in x as the part
# that both tiles cover less 12 columns (its boxes end inside the chunk along y: zeros beyond those ends).
def _long_y(dtype):
    sims, params, union, sigmas, kw = _grid(2, dtype, (1, 2), (1760, 40), (0, 12), SEEDS["long_y"], (2.0, 4.0), trim=8)
    return sims, params, fo.bb([13.0, union["origin"][1]], np.ones(2), (1734, int(union["shape"][1]))), sigmas, kw


def _mid_y(dtype):
    sims, params, union, sigmas, kw = _grid(2, dtype, (1, 2), (1600, 72), (0, 52), SEEDS["mid_y"], (2.0, 4.0), trim=8)
    return sims, params, fo.bb([union["origin"][0], 34.0], np.ones(2), (int(union["shape"][0]), 24)), sigmas, kw


def _stray_views(dtype):
    """A (1, 2, 2) grid of 4 planes (z extent below the second radius) and two more views with the first tile's voxels: one far off
    in y, one whose first row (coordinate 0.4) lies on the last row of the chunk."""
    sims, params, out_bb, sigmas, kw = _grid(3, dtype, (1, 2, 2), (4, 40, 44), (0, 12, 14), SEEDS["stray_views"], (1.0, 2.0))
    first = np.asarray(sims[0].data)
    last_row = out_bb["origin"][1] + (int(out_bb["shape"][1]) - 1)
    for shift in ([0.3, 500.25, 10.5], [0.3, last_row - 0.4, 10.5]):
        sims.append(ac._tile(first, np.ones(3), np.zeros(3)))
        p = np.eye(4)
        p[:3, 3] = shift
        params.append(p)
    return sims, params, out_bb, sigmas, kw


@functools.lru_cache(maxsize=None)
def _build(name, dtype):
    if name == "lightsheet_pair":
        return _lightsheet_pair(dtype)
    if name in ROTATED:
        sims, params, out_bb, kw = ac.build(name, dtype)
        return list(sims), list(params), out_bb, (1.0, 2.0), kw
    seed = SEEDS[name]
    if name == "short_z3":
        return _grid(3, dtype, (1, 2, 2), (3, 40, 44), (0, 12, 14), seed, (1.5, 3.0))
    if name == "short_z7":
        return _grid(3, dtype, (1, 2, 2), (7, 40, 44), (0, 12, 14), seed, (1.5, 3.0))
    if name == "one_plane":
        return _one_plane(dtype)
    if name == "short_z_default":
        return _grid(3, dtype, (1, 2, 2), (30, 40, 44), (0, 12, 14), seed, (5.0, 11.0))
    if name == "short_y_2d":
        return _grid(2, dtype, (1, 2), (9, 60), (0, 16), seed, (1.5, 3.0))
    if name == "stray_views":
        return _stray_views(dtype)
    if name == "radius_128":
        return _grid(2, dtype, (2, 2), (150, 160), (40, 44), seed, (5.0, 32.0), trim=64)
    if name == "long_y":
        return _long_y(dtype)
    if name == "mid_y":
        return _mid_y(dtype)
    if name == "nine_views_3d":
        return _grid(3, dtype, (1, 3, 3), (10, 40, 44), (0, 12, 14), seed, (1.0, 2.0))
    raise KeyError(name)


def build(name, dtype=np.uint16):
    """The case ``name`` with tiles of ``dtype``: (sims, params, out_bb, sigmas, kwargs).  Built once; leave it unchanged."""
    return _build(name, np.dtype(dtype))


def sigma_kwargs(sigmas):
    return {"sigma_1": float(sigmas[0]), "sigma_2": float(sigmas[1])}


def effective_noise_floor(dbg, fused_f, sigmas):
    """``helpers.reference_noise_floor`` of a content-based chunk.  The additive weight of a view is its blending weight times its
    normalised content weight Fn <= 1 (``fo.content_based`` of the oracle's own views and normalised weights), so the absolute noise
    eps_w of the cosine ramp stands against raw_w * Fn where the plain fusion has raw_w: the same bound with that weight in its
    place.  A derivation, not a measured number."""
    fn = fo.content_based(dbg["views"], fo.normalize_weights(dbg["raw_weights"]), *sigmas)
    return reference_noise_floor(dict(dbg, raw_weights=dbg["raw_weights"] * np.nan_to_num(fn)), fused_f)


@functools.lru_cache(maxsize=None)
def _oracle(name, dtype, order):
    sims, params, out_bb, sigmas, kw = _build(name, dtype)
    views, bbs = zip(*[sim_to_view(s) for s in sims])
    fused, fused_f, dbg = fo.fuse_np(list(views), list(params), out_bb, weights="content_based", weights_kwargs=sigma_kwargs(sigmas),
                                     full_view_bbs=list(bbs), interpolation_order=order, return_debug=True, **kw)
    return fused, fused_f, dbg, effective_noise_floor(dbg, fused_f, sigmas)


def oracle(name, dtype=np.uint16, order=1):
    """``fo.fuse_np(..., weights="content_based", return_debug=True)`` of a case and its noise floor: (fused, fused float32, debug,
    floor).  Computed once; leave it unchanged."""
    return _oracle(name, np.dtype(dtype), order)


# ---- csrc/mvs_cb_plan.h, restated: integers only ----
K_GAUSS, LDS_BUDGET, MAX_RADIUS, NEAR_CAP = 8, 60 * 1024, 127, 256


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def _pair_fits(n, r, T):
    return (n + 2 * r) * (T + 1) * 8 <= LDS_BUDGET


def pair_T(n, r, axis):
    T = 8 if axis == 2 else 16
    while T > 1 and not _pair_fits(n, r, T):
        T >>= 1
    return 0 if (not _pair_fits(n, r, T) or (axis != 2 and T < 4)) else T


def single_T(n, r, axis):
    lds = lambda T: (n + 2 * r) * (T + 1) * 4
    T = 8 if axis == 2 else 32
    while T > 1 and lds(T) > LDS_BUDGET:
        T >>= 1
    return T if (lds(T) <= LDS_BUDGET and (axis == 2 or T >= 8)) else 0


def _fast_lds(n, r, T, pf):
    rows = n + 2 * r + K_GAUSS
    if not pf:
        return rows * (T + 1) * 4
    s8 = (rows + 7) // 8 + 1
    s8 += (12 - (s8 & 7)) & 7
    return T * (8 * s8 + 11) * 4 + NEAR_CAP * T * 4


def fast_line_fits(n, r, axis):
    """cb_fast_view_T != 0: the smallest admissible T fits the budget (larger ones are only preferred)."""
    return n <= 0 or _fast_lds(n, r, 8 if axis == 2 else 32, axis == 2) <= LDS_BUDGET


def view_boxes(name):
    """Per view the extents (3, leading ones for 2D) of the bounding box of its in-bounds voxels in the chunk, from the oracle's
    resampled uint16 views (NaN = out of bounds); zeros for a view that does not reach the chunk.  A translated view's box in
    csrc/mvs_gauss.hip is exactly this; a turned view's is the clipped bounding box of its mapped slab, which holds it."""
    views = oracle(name, U16)[2]["views"]
    out = []
    for v in views:
        inb = ~np.isnan(v)
        inb = inb.reshape((1,) * (3 - inb.ndim) + inb.shape)
        if not inb.any():
            out.append((0, 0, 0))
            continue
        idx = np.argwhere(inb)
        out.append(tuple(int(n) for n in idx.max(0) - idx.min(0) + 1))
    return out


def pixel_matrices(name):
    from multiview_stitcher_amd import transformation

    sims, params, out_bb, _, _ = build(name, U16)
    out = []
    for s, p in zip(sims, params):
        view, bb = sim_to_view(s)
        out.append(transformation.get_pixel_affine(np.linalg.inv(p), view["origin"], bb["spacing"], out_bb["origin"], out_bb["spacing"])[0])
    return out


def plan(name):
    """What csrc/mvs_cb_plan.h decides for a case: ``reasons`` -- every check of the default path that declines the chunk, in the
    header's order -- and the counters of the bit-faithful passes that run instead (per view with a box 2 * ndim paired line launches, or
    4 * ndim separate ones, each LDS-staged or tap by tap)."""
    sims, _, out_bb, sigmas, _ = build(name, U16)
    ndim, nv = len(out_bb["shape"]), len(sims)
    cs = (1,) * (3 - ndim) + tuple(int(n) for n in out_bb["shape"])
    r1, r2 = radius(sigmas[0]), radius(sigmas[1])
    axes = range(3 - ndim, 3)
    boxes = view_boxes(name)
    identity = all(np.array_equal(m, np.eye(ndim)) for m in pixel_matrices(name))
    reasons = []
    if nv > 8:
        reasons.append("kCbViewCount")
    if any(cs[a] < max(r1, r2) for a in axes):
        reasons.append("kCbShortAxis")
    if not identity:
        reasons.append("kCbMatrix")
    if max(r1, r2) > MAX_RADIUS:
        reasons.append("kCbRadius")
    if not all(fast_line_fits(b[a], r, a) for b in boxes for a in axes for r in (r1, r2)):
        reasons.append("kCbLine")
    live = [b for b in boxes if b[0] * b[1] * b[2] > 0]
    paired = all(pair_T(b[a], r, a) for b in live for a in axes for r in (r1, r2))
    counters = {"cb_exact_chunks": 1, "cb_exact_large_chunks": int(nv > 8), "cb_exact_paired_launches": 0, "cb_exact_lds_launches": 0,
                "cb_exact_tap_launches": 0}
    if paired:
        counters["cb_exact_paired_launches"] = 2 * ndim * len(live)
    else:
        for b in live:
            for r in (r1, r2):
                for a in axes:          # value and mask: two arrays per filter
                    counters["cb_exact_lds_launches" if single_T(b[a], r, a) else "cb_exact_tap_launches"] += 2
    return {"reasons": reasons, "counters": counters, "boxes": boxes, "chunk": cs, "radii": (r1, r2)}
