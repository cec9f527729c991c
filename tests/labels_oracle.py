"""Plain numpy restatement of label stitching (multiview_stitcher_amd/labels.py, csrc/mvs_labels.hip), written from the stated
definitions and not from the kernels: the voxel counts of a tile, the co-occurrence table of a pair, the matching of labels into
objects and the fusion of the tiles through look-up tables.  Every result is an integer: the kernels must equal it.

Coordinates are float64 in the operation order ``c_k = ((M_k0 p_z + M_k1 p_y) + M_k2 p_x) + o_k`` (2-D: ``(M_k0 p_y + M_k1 p_x) +
o_k``), one numpy operation per step, so nothing is contracted.  A view is in bounds at ``p`` when ``0 <= c_k <= n_k - 1`` on every
axis; its voxel is ``floor(c + 0.5)``."""
import numpy as np


def pixel_affine(p, input_origin, input_spacing, output_origin, output_spacing):
    """(matrix, offset) from a pixel index of the output grid to a pixel coordinate of the input, ``p`` the affine from the output's
    physical space to the input's: matrix = Sy^-1 M Sx, offset = Sy^-1 (t + (M - I) Ox - (Oy - Ox)), rounded to 10 decimals, offsets
    within 1e-6 of an integer snapped to it."""
    p = np.asarray(p, dtype=np.float64)
    ndim = p.shape[0] - 1
    M, t = p[:ndim, :ndim], p[:ndim, ndim]
    sx, sy = np.asarray(output_spacing, dtype=np.float64), np.asarray(input_spacing, dtype=np.float64)
    Ox, Oy = np.asarray(output_origin, dtype=np.float64), np.asarray(input_origin, dtype=np.float64)
    matrix = np.around((M * sx[None, :]) / sy[:, None], decimals=10)
    offset = np.around(((t + np.dot(M - np.eye(ndim), Ox)) - (Oy - Ox)) / sy, decimals=10)
    nearest = np.round(offset)
    snap = np.abs(offset - nearest) <= 1e-6
    offset[snap] = nearest[snap]
    return matrix, offset


def coordinates(matrix, offset, shape, origin=None):
    """c (ndim, *shape) of every index p of a grid of ``shape`` whose first voxel has the index ``origin``."""
    ndim = len(shape)
    origin = [0] * ndim if origin is None else origin
    grid = np.meshgrid(*[np.arange(int(n), dtype=np.float64) + float(o) for n, o in zip(shape, origin)], indexing="ij")
    out = []
    for k in range(ndim):
        c = grid[0] * matrix[k][0]
        c = c + grid[1] * matrix[k][1]
        if ndim == 3:
            c = c + grid[2] * matrix[k][2]
        out.append(c + offset[k])
    return np.stack(out)


def in_bounds(c, shape):
    ok = np.ones(c.shape[1:], dtype=bool)
    for k, n in enumerate(shape):
        ok &= (c[k] >= 0.0) & (c[k] <= float(n - 1))
    return ok


def nearest_voxels(c):
    return tuple(np.floor(c[k] + 0.5).astype(np.int64) for k in range(c.shape[0]))


def label_counts(tile):
    """n[l], l = 0 .. max(label, 0): negative labels are background."""
    return np.bincount(np.maximum(np.asarray(tile).astype(np.int64), 0).ravel()).astype(np.uint64)


def pair_table(A, B, matrix, offset):
    """(la, lb, n) sorted by (la, lb): over every voxel p of A at which B is in bounds, the pairs (max(A[p], 0), max(B[q], 0)) that
    are not (0, 0)."""
    A, B = np.asarray(A).astype(np.int64), np.asarray(B).astype(np.int64)
    c = coordinates(matrix, offset, A.shape)
    ok = in_bounds(c, B.shape)
    q = tuple(i[ok] for i in nearest_voxels(c))
    la, lb = np.maximum(A[ok], 0), np.maximum(B[q], 0)
    keep = (la | lb) != 0
    keys, n = np.unique((la[keep] << 32) | lb[keep], return_counts=True)
    return (keys >> 32).astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32), n.astype(np.uint64)


def match_labels(counts, overlaps, criterion="iou", threshold=0.5, min_voxels=1):
    """(luts, n_objects): the connected components of the (view, label) nodes under the edges whose score reaches the threshold,
    numbered in ascending order of their smallest member."""
    nodes = [(v, l) for v, c in enumerate(counts) for l in range(1, len(c)) if c[l]]
    group = {node: {node} for node in nodes}
    for (a, b), (la, lb, n) in overlaps.items():
        rows = [(int(x), int(y), float(z)) for x, y, z in zip(la, lb, n)]
        a_ov, b_ov = {}, {}
        for x, y, z in rows:
            a_ov[x] = a_ov.get(x, 0.0) + z
            b_ov[y] = b_ov.get(y, 0.0) + z
        for x, y, z in rows:
            if x <= 0 or y <= 0 or z < min_voxels:
                continue
            score = z / (a_ov[x] + b_ov[y] - z) if criterion == "iou" else z / min(a_ov[x], b_ov[y])
            if score >= threshold:
                ga, gb = group[(a, x)], group[(b, y)]
                if ga is not gb:
                    ga |= gb
                    for node in gb:
                        group[node] = ga
    ids = {}
    for node in nodes:                      # ascending (view, label): a component is met first at its smallest member
        if id(group[node]) not in ids:
            ids[id(group[node])] = len(ids) + 1
    luts = [np.zeros(len(c), dtype=np.int32) for c in counts]
    for v, l in nodes:
        luts[v][l] = ids[id(group[(v, l)])]
    return luts, len(ids)


def fuse(tiles, matrices, offsets, luts, out_shape, origin=None):
    """The fused int32 label image: per voxel the view in bounds with the largest d = min over the axes with n_k > 1 of min(c_k,
    (n_k - 1) - c_k), ties to the lowest index; its label through its table (None: the identity), 0 when negative or beyond it."""
    best_d = np.full(out_shape, -1.0)
    out = np.zeros(out_shape, dtype=np.int32)
    for v, (tile, matrix, offset) in enumerate(zip(tiles, matrices, offsets)):
        tile = np.asarray(tile).astype(np.int64)
        c = coordinates(matrix, offset, out_shape, origin)
        d = np.full(out_shape, np.inf)
        for k, n in enumerate(tile.shape):
            if n > 1:
                d = np.minimum(d, np.minimum(c[k], float(n - 1) - c[k]))
        win = in_bounds(c, tile.shape) & (d > best_d)
        label = tile[tuple(i[win] for i in nearest_voxels(c))]
        lut = None if luts is None else luts[v]
        if lut is None:
            value = np.where(label < 0, 0, label)
        else:
            lut = np.asarray(lut).astype(np.int64)
            inside = (label >= 0) & (label < len(lut))
            value = np.where(inside, lut[np.where(inside, label, 0)], 0)
        out[win] = value.astype(np.int32)
        best_d[win] = d[win]
    return out


def same_up_to_bijection(a, b):
    """Is there a one-to-one map of the values of ``a`` onto those of ``b`` that keeps 0 and turns ``a`` into ``b``?"""
    a, b = np.asarray(a).ravel().astype(np.int64), np.asarray(b).ravel().astype(np.int64)
    if a.shape != b.shape or not np.array_equal(a == 0, b == 0):
        return False
    pairs = np.unique(np.stack([a, b]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))
