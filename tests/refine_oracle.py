"""The reference of the sub-pixel refinement tests: lines 74-103 of oracle/reg_oracle.py (``phase_cross_correlation`` up to the
sub-pixel maximum) restated with the working precision as an argument, and returning what that function keeps to itself -- the
refinement array and how far its maximum, and the coarse correlation's, stand above the runner-up.

float64 is the yardstick; float32 (complex64 transforms and kernels, like skimage on float32 images and like the device) is the
restatement whose own distance from the yardstick says what float32 can deliver (tests/test_refine_gpu.py)."""
from collections import namedtuple

import numpy as np
import scipy.fft

from oracle import reg_oracle as ro

Refinement = namedtuple("Refinement", "peak_index coarse_shift refined sub_step coarse_gap refined_gap")


def relative_gap(moduli):
    """(largest - second largest) / largest of an array of moduli."""
    top = np.sort(np.asarray(moduli, dtype=np.float64).ravel())[-2:]
    return float((top[1] - top[0]) / top[1])


def refinement(reference_image, moving_image, upsample_factor, normalization, dtype=np.float64):
    """peak_index: integer arg max of |cc|; coarse_shift: the signed shift rounded to the upsampling grid; refined: the
    ``upsample_factor > 1`` array ``_upsampled_dft(image_product.conj(), ...)`` BEFORE skimage's final ``.conj()`` (what
    mvs_phasecorr_multi_refined hands out; the moduli are the same), U = ceil(1.5 upsample_factor) samples per axis; sub_step: its arg
    max minus the window's centre, in upsampling steps; coarse_gap / refined_gap: ``relative_gap`` of |cc| and of |refined|.  On an axis
    of length 1 the kernel is exactly 1 and all samples along it are equal: the refinement gap is taken over the other axes."""
    dtype = np.dtype(dtype)
    src_freq = scipy.fft.fftn(np.asarray(reference_image).astype(dtype))
    target_freq = scipy.fft.fftn(np.asarray(moving_image).astype(dtype))
    shape = src_freq.shape
    image_product = src_freq * target_freq.conj()
    if normalization == "phase":
        eps = np.finfo(image_product.real.dtype).eps
        image_product /= np.maximum(np.abs(image_product), 100 * eps)
    elif normalization is not None:
        raise ValueError("normalization must be either phase or None")
    cross_correlation = scipy.fft.ifftn(image_product)
    moduli = np.abs(cross_correlation)
    maxima = np.unravel_index(int(np.argmax(moduli)), cross_correlation.shape)
    midpoint = np.array([np.fix(axis_size / 2) for axis_size in shape])
    float_dtype = image_product.real.dtype
    assert float_dtype == dtype
    shift = np.stack(maxima).astype(float_dtype, copy=False)
    shift[shift > midpoint] -= np.array(shape)[shift > midpoint]
    uf = np.array(upsample_factor, dtype=float_dtype)
    shift = np.round(shift * uf) / uf
    upsampled_region_size = np.ceil(uf * 1.5)
    dftshift = np.fix(upsampled_region_size / 2.0)
    sample_region_offset = dftshift - shift * uf
    refined = ro.upsampled_dft(image_product.conj(), [upsampled_region_size] * len(shape), uf, sample_region_offset)
    assert refined.dtype == image_product.dtype
    maxima_u = np.unravel_index(np.argmax(np.abs(refined)), refined.shape)
    sub_step = np.array(maxima_u, dtype=np.int64) - int(dftshift)
    free = tuple(0 if n == 1 else slice(None) for n in shape)
    return Refinement(np.array(maxima), shift, refined, sub_step, relative_gap(moduli), relative_gap(np.abs(refined[free])))
