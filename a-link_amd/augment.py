"""augment — the data augmentation of reference code/helpers.py:114-141 (helpers.augment_data), on the GPU.

The reference appends, per pair and round, the original and three random affine copies of each side:
`tf.contrib.keras.preprocessing.image.random_rotation(x, 20)`, `random_shear(x, 0.2)` and `random_shift(x, 0.2, 0.2)`.
Each draws its parameter from the global np.random stream, builds a 3 x 3 float64 matrix (apply_affine_transform,
transform_matrix_offset_center) and resamples every channel with scipy.ndimage.affine_transform(order=1, mode='nearest').

Here the two halves are split:
  * draw()  takes the same np.random draws in the same order and builds the same matrices with the same np.dot sequence
    (host, float64; a few dozen flops per image);
  * warp()  resamples ANY number of images in one launch of alink_affine_warp (csrc/augment.hip), gathered out of a table
    of source images, with scipy's float64 arithmetic: the float32 pixels equal scipy's bit for bit.

The Keras semantics are those of keras_preprocessing 1.1, what tf.contrib.keras ran under the reference's pinned
tensorflow 1.15: angles and shears in degrees, tx = U(-0.2, 0.2) * H on the row axis, ty = U(-0.2, 0.2) * W on
the column axis, the centre offset float(n) / 2 + 0.5, a byte copy when the drawn parameter is exactly 0.
"""
import collections

import numpy as np

from . import _abi

Plan = collections.namedtuple("Plan", ["src", "maps", "copy", "original"])
Plan.__doc__ = """What draw() returns for R = n * factor * (1 + number of transforms) output rows per side:
    src       (R,) int64         the input row (pair) every output row comes from
    maps      (2, R, 2, 3) f64   per side, the map handed to scipy: (affine matrix | offset) rows
    copy      (2, R) bool        per side, the output is the input untouched (the original, or a parameter drawn as 0)
    original  (R,) bool          the row is the untransformed original (the first of every pair and round)"""


def transform_matrix_offset_center(matrix, x, y):
    """keras_preprocessing.image.affine_transformations.transform_matrix_offset_center, verbatim"""
    o_x = float(x) / 2 + 0.5
    o_y = float(y) / 2 + 0.5
    offset_matrix = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset_matrix = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    transform_matrix = np.dot(np.dot(offset_matrix, matrix), reset_matrix)
    return transform_matrix


def affine_map(h, w, theta=0, tx=0, ty=0, shear=0):
    """The matrix part of keras_preprocessing's apply_affine_transform (no zoom): the (2, 3) map scipy receives, or None
    when every parameter is 0 and Keras returns the image untouched"""
    transform_matrix = None
    if theta != 0:
        theta = np.deg2rad(theta)
        transform_matrix = np.array([[np.cos(theta), -np.sin(theta), 0],
                                     [np.sin(theta), np.cos(theta), 0],
                                     [0, 0, 1]])
    if tx != 0 or ty != 0:
        shift_matrix = np.array([[1, 0, tx],
                                 [0, 1, ty],
                                 [0, 0, 1]])
        transform_matrix = shift_matrix if transform_matrix is None else np.dot(transform_matrix, shift_matrix)
    if shear != 0:
        shear = np.deg2rad(shear)
        shear_matrix = np.array([[1, -np.sin(shear), 0],
                                 [0, np.cos(shear), 0],
                                 [0, 0, 1]])
        transform_matrix = shear_matrix if transform_matrix is None else np.dot(transform_matrix, shear_matrix)
    if transform_matrix is None:
        return None
    transform_matrix = transform_matrix_offset_center(transform_matrix, h, w)
    return np.concatenate([transform_matrix[:2, :2], transform_matrix[:2, 2:3]], axis=1)


def draw(n, H, W, factor=1, use_random_rotation=True, use_random_shear=True, use_random_shift=True):
    """The np.random draws of helpers.augment_data over n pairs of H x W images, in the reference's order — per pair and
    round: rotation left, right; shear left, right; shift left (tx, ty), right (tx, ty) — and the maps they make.
    All draws are taken in one random_sample call and mapped as low + (high - low) * r: the same doubles as the scalar
    np.random.uniform calls, and the same stream state afterwards.  Returns a Plan."""
    kinds = ["original"] + [k for k, on in (("rotation", use_random_rotation), ("shear", use_random_shear),
                                           ("shift", use_random_shift)) if on]
    per_round = 2 * bool(use_random_rotation) + 2 * bool(use_random_shear) + 4 * bool(use_random_shift)
    rounds = int(n) * int(factor)
    R = rounds * len(kinds)
    draws = np.random.random_sample(rounds * per_round).reshape(rounds, per_round) if rounds * per_round else \
        np.zeros((rounds, 0))
    src = np.repeat(np.arange(int(n), dtype=np.int64), int(factor) * len(kinds))
    maps = np.zeros((2, R, 2, 3))
    maps[:, :, 0, 0] = maps[:, :, 1, 1] = 1.0
    copy = np.zeros((2, R), bool)
    original = np.zeros(R, bool)

    def uniform(low, high, r):
        return low + (high - low) * r

    for j in range(rounds):
        d, t = draws[j], 0
        for kk, kind in enumerate(kinds):
            row = j * len(kinds) + kk
            for s in (0, 1):
                if kind == "original":
                    m = None
                elif kind == "rotation":
                    m = affine_map(H, W, theta=uniform(-20, 20, d[t]))
                    t += 1
                elif kind == "shear":
                    m = affine_map(H, W, shear=uniform(-0.2, 0.2, d[t]))
                    t += 1
                else:
                    tx = uniform(-0.2, 0.2, d[t]) * H
                    ty = uniform(-0.2, 0.2, d[t + 1]) * W
                    m = affine_map(H, W, tx=tx, ty=ty)
                    t += 2
                if m is None:
                    copy[s, row] = True
                else:
                    maps[s, row] = m
            original[row] = kind == "original"
    return Plan(src, maps, copy, original)


def warp(table, src, maps, order=1, copy=None):
    """scipy.ndimage.affine_transform(channel, maps[i][:, :2], maps[i][:, 2], order, mode='nearest') on every channel of
    table[src[i]], for all i in ONE launch (alink_affine_warp).  table: (n_in, H, W, C) float images, a NumPy array or a
    CUDA tensor (NumPy in -> NumPy out, CUDA tensor in -> CUDA tensor out, on the table's device); src: (R,) row indices
    into the table, or None for 0 .. R - 1; maps: (R, 2, 3); copy: optional (R,) bool, rows that are byte copies of their
    source.  Returns (R, H, W, C) float32."""
    import torch
    as_torch = isinstance(table, torch.Tensor)
    if as_torch:
        if not table.is_cuda:
            raise ValueError("warp: a torch table must live on a GPU")
        x = table.to(torch.float32).contiguous()
    else:
        x = np.ascontiguousarray(np.asarray(table), dtype=np.float32)
    if x.ndim != 4:
        raise ValueError("warp: expected a table of shape (n, H, W, C), got %s" % (tuple(x.shape),))
    n_in, H, W, Cc = (int(v) for v in x.shape)
    maps = np.ascontiguousarray(np.asarray(maps, dtype=np.float64))
    R = len(maps)
    if maps.shape != (R, 2, 3):
        raise ValueError("warp: maps must be (R, 2, 3), got %s" % (maps.shape,))
    if src is not None:
        src = np.asarray(src.detach().cpu() if hasattr(src, "detach") else src).astype(np.int64).reshape(-1)
        if len(src) != R:
            raise ValueError("warp: %d source rows for %d maps" % (len(src), R))
        if R and (src.min() < 0 or src.max() >= n_in):
            raise IndexError("warp: source row out of range [0, %d)" % n_in)
    elif R > n_in:
        raise ValueError("warp: %d maps for a table of %d images and no source rows" % (R, n_in))
    if copy is not None:
        copy = np.asarray(copy, dtype=bool).reshape(-1)
        if len(copy) != R:
            raise ValueError("warp: %d copy flags for %d maps" % (len(copy), R))
    if order not in (0, 1):
        raise ValueError("warp: order must be 0 or 1, got %r" % (order,))
    if R == 0:
        return x.new_zeros((0, H, W, Cc)) if as_torch else np.zeros((0, H, W, Cc), np.float32)
    device = x.device.index if as_torch else _abi.resolve_device(None)
    lib = _abi.init(device)
    dev = torch.device("cuda", device)
    if not as_torch:
        x = torch.from_numpy(x).to(dev)
    out = torch.empty((R, H, W, Cc), dtype=torch.float32, device=dev)
    d_mat = torch.from_numpy(maps).to(dev)
    d_src = torch.from_numpy(src.astype(np.int32)).to(dev) if src is not None else None
    d_copy = torch.from_numpy(copy.astype(np.uint8)).to(dev) if copy is not None else None
    _abi.check(lib.alink_affine_warp(_abi.ptr(x), n_in, _abi.ptr(d_src), _abi.ptr(d_mat), _abi.ptr(d_copy), R, H, W, Cc,
                                     int(order), _abi.ptr(out), _abi.current_stream(device)), "alink_affine_warp")
    return out if as_torch else out.cpu().numpy()
