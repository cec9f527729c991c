"""Regenerate dct_weights_ref.npz: outputs of the reference's weights.content_based_dct on the seeded cases of
tests/dct_oracle.py (inputs are rebuilt from the seeds, only outputs are stored).

    python tests/golden/make_dct_weights_fixture.py <path to the reference's src/multiview_stitcher/weights.py>

The module imports xarray and a few package modules it does not use on this path; small stand-ins are registered
for them, and the module is imported by path.  Its first normalize_weights call receives the shifted quality
grids (Q - nanmin(Q)); they are recorded through a wrapper."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import dct_oracle as do  # noqa: E402


def _stubs():
    xr = types.ModuleType("xarray")
    xr.DataArray = type("DataArray", (), {})
    pkg = types.ModuleType("multiview_stitcher")
    pkg.__path__ = []
    misc = types.ModuleType("multiview_stitcher.misc_utils")

    def requires_overlap(fn):
        import inspect

        def deco(func):
            defaults = {k: v.default for k, v in inspect.signature(func).parameters.items() if v.default is not inspect.Parameter.empty}
            func.required_overlap = lambda kw: fn({**defaults, **(kw or {})})
            return func

        return deco

    misc.requires_overlap = requires_overlap
    misc.clear_cupy_memory = lambda: None
    sys.modules.update({
        "xarray": xr, "multiview_stitcher": pkg, "multiview_stitcher.misc_utils": misc,
        "multiview_stitcher.spatial_image_utils": types.ModuleType("multiview_stitcher.spatial_image_utils"),
        "multiview_stitcher.transformation": types.ModuleType("multiview_stitcher.transformation"),
    })
    pkg.misc_utils = misc
    pkg.spatial_image_utils = sys.modules["multiview_stitcher.spatial_image_utils"]
    pkg.transformation = sys.modules["multiview_stitcher.transformation"]


def main(ref_path):
    _stubs()
    spec = importlib.util.spec_from_file_location("ref_weights", ref_path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    plain = ref.normalize_weights
    seen = []

    def recording(w):
        seen.append(np.array(w, copy=True))
        return plain(w)

    ref.normalize_weights = recording
    out = {}
    for name, (views, kw) in do.cases().items():
        seen.clear()
        out[f"w/{name}"] = ref.content_based_dct(views, **kw).astype(np.float32)
        out[f"qs/{name}"] = seen[0].astype(np.float32)
    for i, (kw, ocs) in enumerate(do.overlap_cases()):
        ov = ref.content_based_dct.required_overlap(dict(kw, output_chunksize=ocs))
        out[f"overlap/{i}"] = np.array([ov[d] for d in sorted(ov)], np.int64)
    np.savez_compressed(os.path.join(HERE, "dct_weights_ref.npz"), **out)
    print(len(out), "entries")


if __name__ == "__main__":
    main(sys.argv[1])
