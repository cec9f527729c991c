"""A/B of fusion.fuse's host driver between two source trees, without a GPU: fusion.fuse_np is replaced by a recording
stand-in, so what is compared is what the driver DECIDES -- which blocks exist, what each fuse_np call receives, where its
result lands, what ends up in a store -- not voxels.

  python tools/fuse_driver_ab.py dump OUT.txt [--tree ROOT]     one line per fuse_np call, result and store digests
  python tools/fuse_driver_ab.py time [--tree ROOT] [--reps N]  ms per fuse() call of the driver alone (JSON line)

Run ``dump`` once per tree (``--tree``: repository root whose package is imported; default: this file's) and compare the two
files byte for byte; run ``time`` alternating between the trees.  profiles/fuse_driver_ab.txt records an outcome."""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time
import warnings

import numpy as np


def _digest(v):
    """Stable text for any argument value fuse_np receives."""
    if isinstance(v, dict):
        return "{" + ",".join(f"{k}:{_digest(x)}" for k, x in v.items()) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(_digest(x) for x in v) + "]"
    if isinstance(v, np.ndarray):
        return f"nd{v.shape}{v.dtype}:" + hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest()[:12]
    if hasattr(v, "dims") and hasattr(v, "coords"):      # a slab: its shape, its coordinates, the voxels it selected
        return "sim(" + ",".join(f"{d}={len(v.coords[d])}@{_digest(np.asarray(v.coords[d], dtype=float))}" for d in v.dims) + \
            ";" + _digest(np.asarray(v.data)) + ")"
    if callable(v):
        return getattr(v, "__name__", repr(type(v)))
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    if isinstance(v, (int, np.integer)):
        return repr(int(v))
    return repr(v)


def _store_lines(url):
    out = []
    for root, _, files in sorted(os.walk(url)):
        for f in sorted(files):
            p = os.path.join(root, f)
            out.append(f"  file {os.path.relpath(p, url)} {hashlib.sha1(open(p, 'rb').read()).hexdigest()[:12]}")
    return out


class StandIn:
    """fuse_np that records its keyword arguments and returns the block filled with (call index mod 250) + 1."""

    def __init__(self, log=None):
        self.log, self.n = log, 0

    def __call__(self, **kw):
        self.n += 1
        sims, op = kw["sims"], kw["output_properties"]
        trim = kw.get("trim_overlap_in_pixels", 0)
        shape = tuple(int(op["shape"][d]) - 2 * int(trim[d] if isinstance(trim, dict) else trim) for d in op["shape"])
        if self.log is not None:
            self.log.append(f"  call {self.n} " + " ".join(f"{k}={_digest(kw[k])}" for k in sorted(kw)))
        return np.full(shape, (self.n - 1) % 250 + 1, dtype=sims[0].dtype)


def _custom_fusion(transformed_views, blending_weights):
    return np.nansum(transformed_views * blending_weights, axis=0)


def configurations(pkg, tmp):
    """[(name, make)]; ``make()`` -> (images, fuse kwargs).  Built lazily: stores are written when the configuration runs."""
    fusion, sample_data, si, msi_utils, ngff_utils = pkg.fusion, pkg.sample_data, pkg.spatial_image_utils, pkg.msi_utils, pkg.ngff_utils
    key = sample_data.METADATA_TRANSFORM_KEY

    def mosaic(ndim, shift=None, jitter=0):
        if ndim == 3:
            sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=(16, 40, 48), tiles=(1, 2, 2), overlap=(0, 8, 10), max_jitter=jitter)
        else:
            sims, _, _ = sample_data.generate_tiled_dataset(ndim=2, tile_shape=(40, 48), tiles=(2, 2), overlap=(8, 10), max_jitter=jitter)
        if shift is not None:
            p = np.eye(ndim + 1)
            p[:ndim, ndim] = shift[-ndim:]
            si.set_sim_affine(sims[1], p, key)
        return sims

    def fields(ndim):
        rng = np.random.default_rng(3)
        sp = (6, 30, 36)[-ndim:]
        sdims = ["z", "y", "x"][-ndim:]
        sims = []
        for tr in ([0.0, 0.0, 0.0], [0.0, 3.0, 20.0]):
            sim = si.get_sim_from_array(rng.integers(0, 4000, (2, 3) + sp).astype(np.uint16), dims=["c", "t"] + sdims,
                                        translation=dict(zip(sdims, tr[-ndim:])), transform_key=key)
            sims.append(sim)
        p = np.stack([np.eye(ndim + 1)] * 3)
        p[:, ndim - 1, ndim] = [0.0, 7.0, 15.0]      # the second view moves along x with t
        si.set_sim_affine(sims[1], p, key)
        return sims

    def zarr_in(ndim):
        out = []
        for i, s in enumerate(mosaic(ndim)):
            url = os.path.join(tmp, f"in{ndim}_{i}.zarr")
            if not os.path.exists(url):
                ngff_utils.write_sim_to_ome_zarr(s, url)
            z = ngff_utils.read_sim_from_ome_zarr(url)
            z.attrs["transforms"] = dict(s.attrs["transforms"])
            out.append(z)
        return out

    def rotated(ndim):
        sims = mosaic(ndim)
        a = np.deg2rad(7.0)
        p = np.eye(ndim + 1)
        p[ndim - 2:ndim, ndim - 2:ndim] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        si.set_sim_affine(sims[2], p, key)
        return sims

    def planes():
        # output planes on the views' z grid with chunks one plane thick: plane-wise blocks
        sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=(4, 20, 24), tiles=(1, 1, 2), overlap=(0, 0, 6), max_jitter=0)
        return sims

    def msims(ndim):
        shape = (8, 220, 260)[-ndim:]
        rng = np.random.default_rng(1)
        sdims = ["z", "y", "x"][-ndim:]
        out = []
        for tr in (0.0, 200.0):
            sim = si.get_sim_from_array(rng.integers(0, 4000, shape).astype(np.uint16), dims=sdims,
                                        translation={d: (tr if d == "x" else 0.0) for d in sdims}, transform_key=key)
            out.append(msi_utils.get_msim_from_sim(sim, scale_factors=[{d: (2 if d != "z" else 1) for d in sdims}]))
        return out

    url = lambda name: os.path.join(tmp, name)
    cs = {2: {"y": 16, "x": 16}, 3: {"z": 8, "y": 16, "x": 16}}
    cfgs = []
    add = lambda name, make: cfgs.append((name, make))
    for nd in (2, 3):
        n = f"{nd}d"
        add(f"{n} default merged", lambda nd=nd: (mosaic(nd), {}))
        add(f"{n} requested grid", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], merge_chunks=False)))
        add(f"{n} requested grid fractional shift", lambda nd=nd: (mosaic(nd, [0.0, 0.5, -1.25]), dict(output_chunksize=cs[nd], merge_chunks=False)))
        add(f"{n} small launch budget", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], _max_launch_bytes=20_000)))
        add(f"{n} rotated view order 0", lambda nd=nd: (rotated(nd), dict(output_chunksize=cs[nd], merge_chunks=False, interpolation_order=0)))
        add(f"{n} content_based", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], weights_func=fusion.content_based,
                                                                  weights_func_kwargs={"sigma_1": 1, "sigma_2": 2})))
        add(f"{n} max_fusion by name", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], fusion_func="max")))
        add(f"{n} chunk_filter", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], chunk_filter=lambda bi: sum(bi) % 2 == 0)))
        add(f"{n} overlap trimmed", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], overlap_in_pixels=3)))
        add(f"{n} overlap untrimmed", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], overlap_in_pixels={d: 2 + i for i, d in enumerate(cs[nd])},
                                                                      trim_overlap=False)))
        add(f"{n} custom fusion_func", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], fusion_func=_custom_fusion)))
        add(f"{n} deconvolution", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], fusion_func=fusion.multi_view_deconvolution)))
        add(f"{n} content_based_dct", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], weights_func=fusion.content_based_dct)))
        add(f"{n} caller frame_origin", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], merge_chunks=False,
                                                                        frame_origin=dict(zip(cs[nd], (-3.0, -2.0, -1.0)[-nd:])))))
        add(f"{n} output spacing and origin", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], output_spacing={d: 1.5 for d in cs[nd]},
                                                                              output_origin={d: -4.0 for d in cs[nd]})))
        add(f"{n} intersection mode", lambda nd=nd: (mosaic(nd), dict(output_stack_mode="intersection")))
        add(f"{n} sims alias", lambda nd=nd: ("sims", dict(sims=mosaic(nd))))
        add(f"{n} fields", lambda nd=nd: (fields(nd), dict(output_chunksize=cs[nd], merge_chunks=False)))
        add(f"{n} fields merged", lambda nd=nd: (fields(nd), {}))
        add(f"{n} zarr inputs", lambda nd=nd: (zarr_in(nd), dict(output_chunksize=cs[nd])))
        add(f"{n} zarr inputs requested grid", lambda nd=nd: (zarr_in(nd), dict(output_chunksize=cs[nd], merge_chunks=False)))
        for label, zo in (("v2", {}), ("ome 0.4", {"ome_zarr": True}), ("ome 0.5", {"ome_zarr": True, "ngff_version": "0.5"})):
            add(f"{n} zarr out {label}", lambda nd=nd, zo=zo: (mosaic(nd), dict(output_chunksize=cs[nd], output_zarr_url=url("out.zarr"), zarr_options=zo)))
            add(f"{n} zarr out {label} store chunks", lambda nd=nd, zo=zo: (mosaic(nd), dict(
                output_chunksize=cs[nd], output_zarr_url=url("out.zarr"),
                zarr_options=dict(zo, zarr_array_creation_kwargs={"chunks": [8] * nd}))))
            add(f"{n} zarr out {label} full-rank store chunks", lambda nd=nd, zo=zo: (fields(nd), dict(
                output_chunksize=cs[nd], output_zarr_url=url("out.zarr"),
                zarr_options=dict(zo, zarr_array_creation_kwargs={"chunks": [1, 1] + [8] * nd}))))
        add(f"{n} zarr in and out", lambda nd=nd: (zarr_in(nd), dict(output_chunksize=cs[nd], output_zarr_url=url("out.zarr"))))
        add(f"{n} zarr out no overwrite joins", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], output_zarr_url=url("out.zarr"),
                                                                               zarr_options={"overwrite": False}, _prefill=True)))
        add(f"{n} zarr out chunk_filter", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], output_zarr_url=url("out.zarr"),
                                                                         chunk_filter=lambda bi: bi[-1] % 2 == 0)))
        add(f"{n} batch_options no batch_func", lambda nd=nd: (fields(nd), dict(output_chunksize=cs[nd], output_zarr_url=url("out.zarr"),
                                                                               batch_options={"n_batch": 4})))
        add(f"{n} batch_options batch_func", lambda nd=nd: (mosaic(nd), dict(
            output_chunksize=cs[nd], output_zarr_url=url("out.zarr"), zarr_options={"ome_zarr": True},
            batch_options={"n_batch": 5, "batch_func": _recording_batch_func, "batch_func_kwargs": {"tag": "x"}})))
        add(f"{n} msims", lambda nd=nd: (msims(nd), dict(output_chunksize={d: 64 for d in cs[nd]})))
        add(f"{n} msims zarr out", lambda nd=nd: (msims(nd), dict(output_chunksize={d: 64 for d in cs[nd]}, output_zarr_url=url("out.zarr"))))
        # ---- raising configurations ----
        add(f"{n} error no images", lambda nd=nd: (None, {}))
        add(f"{n} error images and sims", lambda nd=nd: (mosaic(nd), dict(sims=mosaic(nd))))
        add(f"{n} error empty", lambda nd=nd: ([], {}))
        add(f"{n} error zarr with output_on_backend", lambda nd=nd: (mosaic(nd), dict(output_zarr_url=url("out.zarr"), output_on_backend=True)))
        add(f"{n} error backend", lambda nd=nd: (mosaic(nd), dict(backend="numpy")))
        add(f"{n} error mixed kinds", lambda nd=nd: (msims(nd)[:1] + mosaic(nd), {}))
        add(f"{n} error no transform_key", lambda nd=nd: (mosaic(nd), dict(transform_key=None)))
        add(f"{n} error interpolation order", lambda nd=nd: (mosaic(nd), dict(interpolation_order=2)))
        add(f"{n} error stack mode", lambda nd=nd: (mosaic(nd), dict(output_stack_mode="nope")))
        add(f"{n} error singular affine", lambda nd=nd: (mosaic(nd, None), dict(_singular=True)))
        add(f"{n} error untrimmed to zarr", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], overlap_in_pixels=2, trim_overlap=False,
                                                                           output_zarr_url=url("out.zarr"), _prefill=True)))
        add(f"{n} error store chunks rank", lambda nd=nd: (mosaic(nd), dict(output_zarr_url=url("out.zarr"), _prefill=True,
                                                                           zarr_options={"zarr_array_creation_kwargs": {"chunks": [8]}})))
        add(f"{n} error store chunks do not tile", lambda nd=nd: (mosaic(nd), dict(output_chunksize=cs[nd], output_zarr_url=url("out.zarr"), _prefill=True,
                                                                                  zarr_options={"zarr_array_creation_kwargs": {"chunks": [5] * nd}})))
        add(f"{n} error zarr_format conflict", lambda nd=nd: (mosaic(nd), dict(output_zarr_url=url("out.zarr"), _prefill=True, zarr_options={
            "ome_zarr": True, "ngff_version": "0.5", "zarr_array_creation_kwargs": {"zarr_format": 2}})))
        add(f"{n} error unknown batch_options", lambda nd=nd: (mosaic(nd), dict(output_zarr_url=url("out.zarr"), _prefill=True, batch_options={"nbatch": 2})))
        add(f"{n} error batch_options without url", lambda nd=nd: (mosaic(nd), dict(batch_options={"n_batch": 2})))
        add(f"{n} error batch_options with chunk_filter", lambda nd=nd: (mosaic(nd), dict(output_zarr_url=url("out.zarr"),
                                                                                         batch_options={"n_batch": 2}, chunk_filter=lambda bi: True)))
    add("3d plane-wise", lambda: (planes(), dict(output_chunksize={"z": 1, "y": 16, "x": 16})))
    add("3d plane-wise merge off", lambda: (planes(), dict(output_chunksize={"z": 1, "y": 16, "x": 16}, merge_chunks=False)))
    add("3d plane-wise zarr out", lambda: (planes(), dict(output_chunksize={"z": 1, "y": 16, "x": 16}, output_zarr_url=url("out.zarr"))))
    add("3d plane-wise batch_options", lambda: (planes(), dict(output_chunksize={"z": 1, "y": 16, "x": 16}, output_zarr_url=url("out.zarr"),
                                                               batch_options={"n_batch": 3})))
    return cfgs, key


_BATCHES = []


def _recording_batch_func(func, block_ids, tag=None):
    _BATCHES.append(f"  batch tag={tag} {[tuple(int(i) for i in b) for b in block_ids]}")
    for b in block_ids:
        func(b)


def _describe(res, pkg, lines):
    if pkg.msi_utils.is_msim(res):
        for k in pkg.msi_utils.get_sorted_scale_keys(res):
            lines.append(f"  level {k}")
            _describe(res[k], pkg, lines)
        return
    lines.append(f"  result dims={list(res.dims)} data={_digest(np.asarray(res.data))} type={type(res.data).__name__}")
    lines.append("  coords " + " ".join(f"{d}={_digest(np.asarray(res.coords[d]))}" for d in res.dims if d in res.coords))
    lines.append("  transforms " + _digest({k: np.asarray(v) for k, v in res.attrs.get("transforms", {}).items()}))


def run_configuration(pkg, name, make, key, tmp, lines):
    fusion = pkg.fusion
    out_url = os.path.join(tmp, "out.zarr")
    shutil.rmtree(out_url, ignore_errors=True)
    images, kw = make()
    kw = dict(kw)
    if kw.pop("_prefill", False):
        # an existing store: raising configurations show whether it survived, "overwrite: False" joins it
        if "error" in name:
            _write_marker(out_url)
        else:
            shape = _result_shape(pkg, images, key)
            chunks = [1] * (len(shape) - len(kw["output_chunksize"])) + list(kw["output_chunksize"].values())
            pkg.zarr_io.ZarrArray.create(out_url, shape, chunks, np.uint16)
    if kw.pop("_singular", False):
        pkg.spatial_image_utils.set_sim_affine(images[0], np.zeros((len(images[0].dims) - 1,) * 2), key)
    cap = kw.pop("_max_launch_bytes", None)
    kw.setdefault("transform_key", key)
    log = []
    lines.append(f"config {name}")
    stand_in = StandIn(log)
    real, real_cap = fusion.fuse_np, fusion.MAX_LAUNCH_BYTES
    fusion.fuse_np = stand_in
    if cap is not None:
        fusion.MAX_LAUNCH_BYTES = cap
    del _BATCHES[:]
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                res = fusion.fuse(**kw) if isinstance(images, str) or images is None else fusion.fuse(images, **kw)
                outcome = None
            except Exception as exc:      # noqa: BLE001  (the exception IS the outcome that is compared)
                outcome = f"  raised {type(exc).__name__}: {exc}"
        lines.extend(log)
        lines.extend(_BATCHES)
        lines.extend(f"  warning {w.category.__name__}: {w.message}" for w in caught)
        if outcome is not None:
            lines.append(outcome.replace(tmp, "<tmp>"))
        else:
            _describe(res, pkg, lines)
        if os.path.exists(out_url):
            lines.extend(_store_lines(out_url))
    finally:
        fusion.fuse_np, fusion.MAX_LAUNCH_BYTES = real, real_cap
    return stand_in.n


def _write_marker(url):
    os.makedirs(url, exist_ok=True)
    with open(os.path.join(url, "marker"), "w") as f:
        f.write("an existing store")


def _result_shape(pkg, images, key):
    sims = list(images)
    osp = pkg.fusion.process_output_stack_properties(sims, transform_key=key)
    sd = pkg.spatial_image_utils.get_spatial_dims_from_sim(sims[0])
    ns = pkg.spatial_image_utils.get_nonspatial_dims_from_sim(sims[0])
    return [sims[0].sizes[d] for d in ns] + [int(osp["shape"][d]) for d in sd]


def time_driver(pkg, reps):
    """ms per fuse() of the driver alone on a 4 x 4 x 4 mosaic of 40^3 tiles with chunks of 16: the requested grid (several
    hundred blocks) and the default merged call."""
    fusion, sample_data = pkg.fusion, pkg.sample_data
    sims, _, _ = sample_data.generate_tiled_dataset(ndim=3, tile_shape=40, tiles=(4, 4, 4), overlap=8, max_jitter=0)
    key = sample_data.METADATA_TRANSFORM_KEY
    real = fusion.fuse_np
    out = {}
    try:
        for label, kw in (("requested_grid", dict(merge_chunks=False)), ("merged", {})):
            stand_in = StandIn()
            fusion.fuse_np = stand_in
            fusion.fuse(sims, transform_key=key, output_chunksize=16, **kw)      # (warm: imports, library load)
            ms = []
            for _ in range(reps):
                stand_in.n = 0
                t0 = time.perf_counter()
                fusion.fuse(sims, transform_key=key, output_chunksize=16, **kw)
                ms.append((time.perf_counter() - t0) * 1e3)
            out[label] = {"calls": stand_in.n, "ms": [round(v, 3) for v in ms]}
    finally:
        fusion.fuse_np = real
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["dump", "time"])
    ap.add_argument("out", nargs="?")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import multiview_stitcher_amd as pkg
    from multiview_stitcher_amd import fusion, msi_utils, ngff_utils, sample_data, spatial_image_utils, zarr_io  # noqa: F401

    assert os.path.abspath(pkg.fusion.__file__).startswith(os.path.abspath(args.tree)), pkg.fusion.__file__
    if args.mode == "time":
        print(json.dumps(time_driver(pkg, args.reps)))
        return
    tmp = tempfile.mkdtemp(prefix="fuse_driver_ab_")
    try:
        cfgs, key = configurations(pkg, tmp)
        lines, calls = [], 0
        for name, make in cfgs:
            calls += run_configuration(pkg, name, make, key, tmp, lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"{len(cfgs)} configurations, {calls} fuse_np calls, sha1 {hashlib.sha1(open(args.out, 'rb').read()).hexdigest()}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
