"""CPU: the host side of multi-view deconvolution -- the restatement (tests/deconv_oracle.py) and the project's PSF /
compound-kernel helpers against the reference's outputs (tests/golden/mv_deconv_ref.npz), required_overlap, the
rank-1 test, the public names, the C ABI's struct and argument checks (no device needed)."""
import ctypes
import os

import numpy as np
import pytest

from tests import deconv_oracle as do

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mv_deconv_ref.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


@pytest.mark.parametrize("name", sorted(do.cases()))
def test_restatement_equals_reference(ref, name):
    views, blend, kw = do.cases()[name]
    got = do.deconvolve(views, blend, n_iterations=do.FIXTURE_ITERATIONS, **kw)
    want = ref[f"run/{name}"]
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-6 * np.abs(want).max()


def test_psf_helpers_equal_reference(ref):
    from multiview_stitcher_amd import mv_deconv

    for name, (fn, args, kw) in do.helper_cases().items():
        got = getattr(mv_deconv, fn)(*args, **kw)
        want = ref[f"psf/{name}"]
        assert got.dtype == np.float32 and np.array_equal(got, want), name


@pytest.mark.parametrize("psf_type", do.PSF_TYPES)
def test_compound_kernels_equal_reference(ref, psf_type):
    from multiview_stitcher_amd import mv_deconv

    psfs = do.compound_inputs()
    for v in range(len(psfs)):
        for t in (psf_type, mv_deconv.PSFType(psf_type)):
            got = mv_deconv.compound_kernel(v, psfs, t)
            assert got.dtype == np.float32 and np.array_equal(got, ref[f"k2/{psf_type}/{v}"])


def test_required_overlap(ref):
    from multiview_stitcher_amd import fusion

    ro = fusion.multi_view_deconvolution.required_overlap
    assert ro({}) == ro(None) == int(ref["overlap/none"]) == 4
    assert ro({"output_spacing": {"z": 1.0, "y": 1.0, "x": 1.0}}) == int(ref["overlap/spacing1"]) == 5
    assert ro({"output_spacing": {"z": 0.5, "y": 0.1, "x": 0.1}, "na": 1.0}) == int(ref["overlap/spacing_fine"])


def test_rank_one_detection():
    from multiview_stitcher_amd import mv_deconv

    for k in [mv_deconv.make_gaussian_psf(1.5, ndim=3), mv_deconv.estimate_psf({"z": 1.0, "y": 1.0, "x": 1.0}),
              mv_deconv.make_gaussian_psf([1.0, 2.0])]:
        f = mv_deconv.separable_factors(k)
        assert f is not None
        outer = f[0].astype(np.float64)
        for g in f[1:]:
            outer = np.multiply.outer(outer, g)
        assert np.abs(outer - k).max() <= 1e-6 * np.abs(k).max()
    psfs = do.compound_inputs()
    for t in do.PSF_TYPES:
        assert mv_deconv.separable_factors(mv_deconv.compound_kernel(0, psfs, t)) is not None
    assert mv_deconv.separable_factors(do.cases()["2d_nonseparable"][2]["psfs"][0]) is None


def test_public_names_resolve():
    from multiview_stitcher_amd import fusion, mv_deconv

    assert fusion.builtin("multi_view_deconvolution") is fusion.multi_view_deconvolution is mv_deconv.multi_view_deconvolution
    assert fusion.PSFType is mv_deconv.PSFType
    assert [m.value for m in fusion.PSFType] == list(do.PSF_TYPES)
    assert fusion.has_keyword(fusion.multi_view_deconvolution, "blending_weights")
    assert fusion.has_keyword(fusion.multi_view_deconvolution, "output_spacing")
    assert "multi_view_deconvolution" not in fusion._FUSION_CODES


def test_argument_errors_before_any_device():
    from multiview_stitcher_amd import fusion

    views, blend, _ = do.cases()["2d_one_view"]
    with pytest.raises(ValueError):
        fusion.multi_view_deconvolution(views, blend, psfs=[np.ones((3, 3)), np.ones((3, 3))])
    with pytest.raises(NotImplementedError, match="63"):
        fusion.multi_view_deconvolution(views, blend, psfs=[np.ones((3, 65))])


def test_deconv_opts_layout():
    from multiview_stitcher_amd import _lib

    assert ctypes.sizeof(_lib.mvs_deconv_opts_t) == 4 + 4 + 8 + 8 + 24 + 4 + 4
    assert _lib.mvs_deconv_opts_t.trim.offset == 24


def test_abi_refuses_bad_arguments():
    from multiview_stitcher_amd import _lib

    lib = _lib.load()
    C = ctypes
    views = np.zeros((1, 4, 4), np.float32)
    k = np.ones((1, 3, 3), np.float32)
    opts = _lib.mvs_deconv_opts_t()
    opts.n_iterations, opts.min_value, opts.out_dtype = 1, 1e-4, _lib.MVS_F32
    out = np.zeros((4, 4), np.float32)

    def call(shape=(1, 4, 4), ndim=2, ksize=(1, 3, 3), n_views=1, o=opts, kern=k):
        return lib.mvs_mv_deconv(0, views.ctypes.data, views.ctypes.data, n_views, _lib.i64x3(shape), ndim,
                                 None if kern is None else kern.ctypes.data, k.ctypes.data, _lib.i64x3(ksize), None, None,
                                 C.byref(o), out.ctypes.data, _lib.MVS_MEM_HOST)

    assert call(kern=None) == -1
    assert call(n_views=0) == -1
    assert call(ndim=4) == -1
    assert call(shape=(2, 4, 4)) == -1                  # 2D data has one plane
    assert call(shape=(1, 0, 4)) == -1
    assert call(ksize=(1, 3, 64), shape=(1, 4, 4)) == -4   # over the kernel limit: MVS_ERR_UNSUPPORTED
    bad = _lib.mvs_deconv_opts_t()
    bad.n_iterations, bad.out_dtype = 1, 7
    assert call(o=bad) == -1
    bad.out_dtype, bad.trim[1] = _lib.MVS_F32, 2
    assert call(o=bad) == -1                            # the trim leaves nothing
