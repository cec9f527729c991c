"""GPU parity of the two standalone entry points of the fuse path against the oracle:
mvs_resample (transformation.transform_sim -> scipy affine_transform, transformation.py:15-148; also the registration
pre-transform with cval = NaN, registration.py:318-338) and mvs_blend_weights (weights.get_blending_weights,
weights.py:391-511), plus the hand-derived blending ramp of tests/test_weights_oracle.py through the HIP fuse."""
import numpy as np
import pytest
from scipy.ndimage import affine_transform

from oracle import fuse_oracle as fo
from tests.helpers import bb_to_dicts
from tests.test_weights_oracle import two_tile_case

pytestmark = pytest.mark.gpu


def _random_affine(ndim, rng, rot=0.3, scale=0.1, shift=4.0):
    a = np.eye(ndim + 1)
    m = np.eye(ndim) + rng.uniform(-rot, rot, (ndim, ndim))
    m *= 1 + rng.uniform(-scale, scale, ndim)[:, None]
    a[:ndim, :ndim] = m
    a[:ndim, ndim] = rng.uniform(-shift, shift, ndim)
    return a


EXACT_KINDS = ("rot90", "rot270", "mirror", "swap")


def _exact_pixel_affine(kind, shape):
    """Pixel matrix and integer offset of the kinds whose view borders fall on output voxels: a turn in the yx plane by np.pi / 2
    (np.cos leaves 6.1e-17 in the matrix: where the other term of a coordinate is 0 it becomes 6.1e-17 * index, inside) or by
    3 * np.pi / 2 (-1.8e-16: there the coordinate is below 0, outside, for every index but 0), a mirror along x, a swap of y and x.
    Elsewhere the coordinates are exactly 0.0 .. n - 1."""
    ndim, (ny, nx) = len(shape), shape[-2:]
    m, o = np.eye(ndim), np.zeros(ndim)
    if ndim == 3:
        o[0] = -2.0
    if kind in ("rot90", "rot270"):
        a = np.pi / 2 if kind == "rot90" else 3 * np.pi / 2
        m[-2:, -2:] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        o[-2:] = [ny - 1, 0.0] if kind == "rot90" else [0.0, nx - 1]
    elif kind == "mirror":
        m[-1, -1] = -1.0
        o[-2:] = [-3.0, nx - 1 + 4]
    else:
        m[-2:, -2:] = [[0.0, 1.0], [1.0, 0.0]]
        o[-2:] = [0.0, -5.0]
    return m, o


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.uint8])
@pytest.mark.parametrize("kind", ["translation", "integer", "affine", *EXACT_KINDS])
def test_resample_matches_scipy_with_nan_cval(hip_device, ndim, order, dtype, kind):
    from multiview_stitcher_amd import transformation

    rng = np.random.default_rng(ndim * 10 + order)
    shape = (37, 52) if ndim == 2 else (11, 29, 33)
    data = (rng.random(shape) * 200).astype(dtype)
    if dtype == np.float32:
        data[tuple(rng.integers(0, n, 12) for n in shape)] = np.nan          # NaN taps poison like scipy
    in_o, in_s = rng.uniform(-3, 3, ndim), np.array([1.0, 0.8, 1.3][-ndim:])
    out_shape = tuple(int(n * 1.2) for n in shape)
    out_bb = fo.bb(in_o - 2.7, np.array([0.9, 1.0, 1.1][-ndim:]), out_shape)
    if kind == "affine":
        p = _random_affine(ndim, rng)
    else:
        p = np.eye(ndim + 1)
        p[:ndim, ndim] = rng.integers(-3, 4, ndim) if kind == "integer" else rng.uniform(-3, 3, ndim)
    if kind == "integer":                                                # same grid, integer pixel offsets
        in_s = np.ones(ndim)
        out_bb = fo.bb(in_o - 2.0, np.ones(ndim), out_shape)
    if kind in EXACT_KINDS:
        # the pixel affine itself, not derived from origins and spacings: that derivation rounds the matrix to 10 decimals
        m, o = _exact_pixel_affine(kind, shape)
        want = affine_transform(data.astype(np.float32), matrix=m, offset=o, output_shape=out_shape, mode="constant", cval=np.nan,
                                order=order)
        assert np.isnan(want).any() and (~np.isnan(want)).mean() > 0.3
    else:
        want = fo.transform_array(data.astype(np.float32), p, in_o, in_s, out_bb, order=order, cval=np.nan)
        m, o = transformation.get_pixel_affine(p, in_o, in_s, out_bb["origin"], out_bb["spacing"])
    got = transformation.resample_array(data, m, o, out_shape, order=order, cval=np.nan)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))        # exact in-bounds classification
    ok = ~np.isnan(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-5, atol=1e-4 * float(np.nanmax(np.abs(want[ok])) if ok.any() else 1))


@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("kind", ["identity", "translation", "affine", "rot90", "mirror", "swap"])
def test_blend_weights_match_oracle(hip_device, ndim, kind):
    from multiview_stitcher_amd import weights

    rng = np.random.default_rng(ndim)
    sd = ["z", "y", "x"][-ndim:]
    shape = (41, 56) if ndim == 2 else (13, 31, 38)
    src = fo.bb(rng.uniform(-2, 2, ndim), np.array([2.0, 1.0, 1.0][-ndim:]), shape)
    tgt = fo.bb(src["origin"] - 3.3, np.array([1.5, 0.9, 1.1][-ndim:]), tuple(int(n * 1.3) for n in shape))
    if kind == "identity":
        p = np.eye(ndim + 1)
    elif kind == "translation":
        p = np.eye(ndim + 1)
        p[:ndim, ndim] = rng.uniform(-4, 4, ndim)
    elif kind == "affine":
        p = _random_affine(ndim, rng, rot=0.2)
    else:
        # unit spacings, origins and offsets whole numbers: the view's borders lie on output voxels
        src = fo.bb(np.zeros(ndim), np.ones(ndim), shape)
        tgt = fo.bb(np.full(ndim, -4.0), np.ones(ndim), tuple(int(n * 1.3) for n in shape))
        p = np.eye(ndim + 1)
        if kind == "rot90":
            p[ndim - 2:ndim, ndim - 2:ndim] = [[np.cos(np.pi / 2), -np.sin(np.pi / 2)], [np.sin(np.pi / 2), np.cos(np.pi / 2)]]
            p[ndim - 2, ndim] = shape[-1] - 1 + 2
        elif kind == "mirror":
            p[ndim - 1, ndim - 1] = -1.0
            p[ndim - 1, ndim] = shape[-1] - 1 + 3
        else:
            p[ndim - 2:ndim, ndim - 2:ndim] = [[0.0, 1.0], [1.0, 0.0]]
            p[ndim - 2:ndim, ndim] = [2.0, -1.0]
    bw = dict(zip(sd, [3.0, 10.0, 6.0][-ndim:]))
    want = fo.get_blending_weights(tgt, src, p, blending_widths=bw)
    got = weights.get_blending_weights(bb_to_dicts(tgt, sd), bb_to_dicts(src, sd), p, blending_widths=bw)
    assert got.dtype == np.float32 and got.shape == want.shape
    np.testing.assert_array_equal(got == 0, want == 0)                  # same support
    np.testing.assert_allclose(got, want, atol=3e-6)


@pytest.mark.parametrize("dtype", [np.float32, np.uint16])
def test_two_tile_fusion_follows_the_hand_derived_ramp(hip_device, dtype):
    """Non-constant tiles: the fused overlap must follow sin^2(pi d / (2 bw)) derived in tests/test_weights_oracle.py."""
    from multiview_stitcher_amd import fusion, spatial_image_utils as si

    n, overlap, bw = 48, 16, 6.0
    views, bbs, out_bb, (a, b, off, wa, wb) = two_tile_case(n, overlap, bw, dtype=dtype)
    sims = [si.to_spatial_image(v["data"], dims=["y", "x"], scale=dict(zip("yx", v["spacing"])), translation=dict(zip("yx", v["origin"])))
            for v in views]
    got = fusion.fuse_np(sims, [np.eye(3), np.eye(3)], bb_to_dicts(out_bb, ["y", "x"]),
                         full_view_bbs=[bb_to_dicts(bbv, ["y", "x"]) for bbv in bbs], blending_widths={"y": bw, "x": bw})
    got = np.asarray(got)
    y = n // 2
    va = np.pad(a[y].astype(np.float64), (0, off))
    vb = np.pad(b[y].astype(np.float64), (off, 0))
    want = (wa * va + wb * vb) / (wa + wb)
    if dtype == np.float32:
        np.testing.assert_allclose(got[y], want, rtol=1e-5)
    else:
        assert np.abs(got[y].astype(np.float64) - np.floor(want)).max() <= 1
