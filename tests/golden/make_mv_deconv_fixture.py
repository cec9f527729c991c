"""Regenerate mv_deconv_ref.npz: outputs of the reference's fusion/mv_deconv.py on the seeded cases of
tests/deconv_oracle.py (inputs are rebuilt from the seeds, only outputs are stored).

    python tests/golden/make_mv_deconv_fixture.py <path to the reference's src/multiview_stitcher/fusion/mv_deconv.py>

The module needs only numpy and scipy; it is imported by path."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import deconv_oracle as do  # noqa: E402


def main(ref_path):
    spec = importlib.util.spec_from_file_location("ref_mv_deconv", ref_path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, (views, blend, kw) in do.cases().items():
        out[f"run/{name}"] = ref.multi_view_deconvolution(views, blend, n_iterations=do.FIXTURE_ITERATIONS, **kw)
    for name, (fn, args, kw) in do.helper_cases().items():
        out[f"psf/{name}"] = getattr(ref, fn)(*args, **kw)
    psfs = do.compound_inputs()
    for t in do.PSF_TYPES:
        for v in range(len(psfs)):
            out[f"k2/{t}/{v}"] = ref._compute_compound_kernel(v, psfs, t)
    out["overlap/none"] = np.int64(ref.multi_view_deconvolution.required_overlap({}))
    out["overlap/spacing1"] = np.int64(ref.multi_view_deconvolution.required_overlap({"output_spacing": {"z": 1.0, "y": 1.0, "x": 1.0}}))
    out["overlap/spacing_fine"] = np.int64(ref.multi_view_deconvolution.required_overlap(
        {"output_spacing": {"z": 0.5, "y": 0.1, "x": 0.1}, "na": 1.0}))
    np.savez_compressed(os.path.join(HERE, "mv_deconv_ref.npz"), **out)
    print(len(out), "entries")


if __name__ == "__main__":
    main(sys.argv[1])
