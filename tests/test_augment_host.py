"""CPU: the host half of helpers.augment_data (a-link_amd/augment.py) against a literal restatement of the Keras functions
the reference calls (code/helpers.py:114-141 -> tf.contrib.keras.preprocessing.image, keras_preprocessing 1.1 under the
reference's tensorflow 1.15): the same np.random draws, the same maps bit for bit, the same stream state afterwards.
The restatement takes the resampler as an argument: scipy.ndimage.affine_transform in tests/test_gpu_augment.py, a
recorder of the maps here."""
import itertools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- keras_preprocessing/image/affine_transformations.py (1.1), restated; only the resampler is a parameter ------------
def transform_matrix_offset_center(matrix, x, y):
    o_x = float(x) / 2 + 0.5
    o_y = float(y) / 2 + 0.5
    offset_matrix = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset_matrix = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    transform_matrix = np.dot(np.dot(offset_matrix, matrix), reset_matrix)
    return transform_matrix


def apply_affine_transform(x, theta=0, tx=0, ty=0, shear=0, zx=1, zy=1, row_axis=0, col_axis=1, channel_axis=2,
                           fill_mode='nearest', cval=0., order=1, resample=ndimage.affine_transform):
    transform_matrix = None
    if theta != 0:
        theta = np.deg2rad(theta)
        rotation_matrix = np.array([[np.cos(theta), -np.sin(theta), 0],
                                    [np.sin(theta), np.cos(theta), 0],
                                    [0, 0, 1]])
        transform_matrix = rotation_matrix
    if tx != 0 or ty != 0:
        shift_matrix = np.array([[1, 0, tx],
                                 [0, 1, ty],
                                 [0, 0, 1]])
        if transform_matrix is None:
            transform_matrix = shift_matrix
        else:
            transform_matrix = np.dot(transform_matrix, shift_matrix)
    if shear != 0:
        shear = np.deg2rad(shear)
        shear_matrix = np.array([[1, -np.sin(shear), 0],
                                 [0, np.cos(shear), 0],
                                 [0, 0, 1]])
        if transform_matrix is None:
            transform_matrix = shear_matrix
        else:
            transform_matrix = np.dot(transform_matrix, shear_matrix)
    if zx != 1 or zy != 1:
        zoom_matrix = np.array([[zx, 0, 0],
                                [0, zy, 0],
                                [0, 0, 1]])
        if transform_matrix is None:
            transform_matrix = zoom_matrix
        else:
            transform_matrix = np.dot(transform_matrix, zoom_matrix)
    if transform_matrix is not None:
        h, w = x.shape[row_axis], x.shape[col_axis]
        transform_matrix = transform_matrix_offset_center(transform_matrix, h, w)
        x = np.rollaxis(x, channel_axis, 0)
        final_affine_matrix = transform_matrix[:2, :2]
        final_offset = transform_matrix[:2, 2]
        channel_images = [resample(x_channel, final_affine_matrix, final_offset, order=order, mode=fill_mode, cval=cval)
                          for x_channel in x]
        x = np.stack(channel_images, axis=0)
        x = np.rollaxis(x, 0, channel_axis + 1)
    return x


def random_rotation(x, rg, row_axis=1, col_axis=2, channel_axis=0, fill_mode='nearest', cval=0., interpolation_order=1,
                    resample=ndimage.affine_transform):
    theta = np.random.uniform(-rg, rg)
    return apply_affine_transform(x, theta=theta, row_axis=row_axis, col_axis=col_axis, channel_axis=channel_axis,
                                  fill_mode=fill_mode, cval=cval, order=interpolation_order, resample=resample)


def random_shift(x, wrg, hrg, row_axis=1, col_axis=2, channel_axis=0, fill_mode='nearest', cval=0., interpolation_order=1,
                 resample=ndimage.affine_transform):
    h, w = x.shape[row_axis], x.shape[col_axis]
    tx = np.random.uniform(-hrg, hrg) * h
    ty = np.random.uniform(-wrg, wrg) * w
    return apply_affine_transform(x, tx=tx, ty=ty, row_axis=row_axis, col_axis=col_axis, channel_axis=channel_axis,
                                  fill_mode=fill_mode, cval=cval, order=interpolation_order, resample=resample)


def random_shear(x, intensity, row_axis=1, col_axis=2, channel_axis=0, fill_mode='nearest', cval=0., interpolation_order=1,
                 resample=ndimage.affine_transform):
    shear = np.random.uniform(-intensity, intensity)
    return apply_affine_transform(x, shear=shear, row_axis=row_axis, col_axis=col_axis, channel_axis=channel_axis,
                                  fill_mode=fill_mode, cval=cval, order=interpolation_order, resample=resample)


# ---- code/helpers.py:114-141, restated over the functions above -----------------------------------------------------
def reference_augment_data(dataset, dataset_labels, augementation_factor=1, use_random_rotation=True, use_random_shear=True,
                           use_random_shift=True, order=1, resample=ndimage.affine_transform):
    kw = dict(row_axis=0, col_axis=1, channel_axis=2, interpolation_order=order, resample=resample)
    augmented_image_left, augmented_image_right, augmented_image_labels = [], [], []
    for num in range(0, dataset[0].shape[0]):
        for i in range(0, augementation_factor):
            augmented_image_left.append(dataset[0][num])
            augmented_image_right.append(dataset[1][num])
            augmented_image_labels.append(dataset_labels[num])
            if use_random_rotation:
                augmented_image_left.append(random_rotation(dataset[0][num], 20, **kw))
                augmented_image_right.append(random_rotation(dataset[1][num], 20, **kw))
                augmented_image_labels.append(dataset_labels[num])
            if use_random_shear:
                augmented_image_left.append(random_shear(dataset[0][num], 0.2, **kw))
                augmented_image_right.append(random_shear(dataset[1][num], 0.2, **kw))
                augmented_image_labels.append(dataset_labels[num])
            if use_random_shift:
                augmented_image_left.append(random_shift(dataset[0][num], 0.2, 0.2, **kw))
                augmented_image_right.append(random_shift(dataset[1][num], 0.2, 0.2, **kw))
                augmented_image_labels.append(dataset_labels[num])
    return [np.array(augmented_image_left), np.array(augmented_image_right)], np.array(augmented_image_labels)


def warp_restated(img, m, order):
    """the float64 arithmetic of csrc/augment.hip on one (H, W) channel and one (2, 3) map"""
    H, W = img.shape
    r = np.arange(H, dtype=np.float64)[:, None]
    c = np.arange(W, dtype=np.float64)[None, :]
    y = np.clip((r * m[0, 0] + c * m[0, 1]) + m[0, 2], 0, H - 1)
    x = np.clip((r * m[1, 0] + c * m[1, 1]) + m[1, 2], 0, W - 1)
    v = img.astype(np.float64)
    if order == 0:
        return (0.0 + v[np.floor(y + 0.5).astype(int), np.floor(x + 0.5).astype(int)]).astype(np.float32)
    y0, x0 = np.floor(y), np.floor(x)
    wy0, wx0 = 1.0 - (y - y0), 1.0 - (x - x0)
    wy1, wx1 = 1.0 - wy0, 1.0 - wx0
    yi, xi = y0.astype(int), x0.astype(int)
    yj, xj = np.minimum(yi + 1, H - 1), np.minimum(xi + 1, W - 1)
    t = 0.0 + v[yi, xi] * wy0 * wx0
    t = t + v[yi, xj] * wy0 * wx1
    t = t + v[yj, xi] * wy1 * wx0
    t = t + v[yj, xj] * wy1 * wx1
    return t.astype(np.float32)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


@pytest.mark.parametrize("factor", [1, 2])
@pytest.mark.parametrize("shape", [(112, 112), (112, 96)])
def test_draw_equals_keras(factor, shape):
    """augment.draw against the Keras functions as helpers.augment_data calls them: every map scipy would receive, bit
    for bit and in order, and the global stream left where the reference leaves it — all 8 use_* combinations"""
    from a_link_amd import augment
    H, W = shape
    n = 3
    for flags in itertools.product((False, True), repeat=3):
        seen = []

        def record(ch, matrix, offset, order, mode, cval):
            assert mode == "nearest" and order == 1
            seen.append(np.concatenate([matrix, np.asarray(offset)[:, None]], axis=1))
            return ch
        x = np.zeros((n, H, W, 1), np.float32)
        np.random.seed(11)
        np.random.random_sample(5)
        reference_augment_data([x, x], np.arange(n), factor, *flags, resample=record)
        want_state = np.random.get_state()
        np.random.seed(11)
        np.random.random_sample(5)
        plan = augment.draw(n, H, W, factor, *flags)
        assert _same_state(np.random.get_state(), want_state), flags
        R = n * factor * (1 + sum(flags))
        assert plan.src.shape == (R,) and plan.maps.shape == (2, R, 2, 3) and plan.copy.shape == (2, R)
        assert np.array_equal(plan.src, np.repeat(np.arange(n), factor * (1 + sum(flags))))
        assert np.array_equal(plan.original, np.tile([True] + [False] * sum(flags), n * factor))
        assert (plan.copy[:, plan.original]).all()
        got = [plan.maps[s, row] for row in range(R) for s in (0, 1) if not plan.copy[s, row]]
        assert len(got) == len(seen) == 2 * n * factor * sum(flags), flags
        for a, b in zip(got, seen):
            assert _bits(a) == _bits(b), (flags, a, b)


def test_a_parameter_drawn_as_zero_is_a_copy(monkeypatch):
    """Keras returns the image untouched when the drawn parameter is 0 (U(-a, a) at r = 0.5): a copy row, no map"""
    from a_link_amd import augment
    monkeypatch.setattr(np.random, "random_sample", lambda k: np.full(k, 0.5))
    plan = augment.draw(2, 32, 32, 1)
    assert plan.copy.all()
    monkeypatch.setattr(np.random, "random_sample", lambda k: np.tile([0.25, 0.5], k // 2))
    plan = augment.draw(1, 32, 32, 1, use_random_rotation=False, use_random_shear=False)
    assert plan.copy.tolist() == [[True, False], [True, False]]        # a shift with tx != 0, ty == 0 still moves the image


def test_warp_arithmetic_equals_scipy():
    """the kernel's float64 arithmetic (restated in NumPy) against scipy.ndimage.affine_transform, order 0 and 1"""
    from a_link_amd import augment
    rng = np.random.RandomState(3)
    for H, W in ((112, 112), (32, 32), (112, 96)):
        img = rng.randint(0, 256, (H, W)).astype(np.float32)
        maps = [augment.affine_map(H, W, theta=rng.uniform(-20, 20)), augment.affine_map(H, W, shear=rng.uniform(-0.2, 0.2)),
                augment.affine_map(H, W, shear=np.rad2deg(0.2)), augment.affine_map(H, W, tx=0.2 * H, ty=-0.13 * W),
                augment.affine_map(H, W, theta=180.0), augment.affine_map(H, W, tx=3.0 * H, ty=-2.0 * W)]
        for m in maps:
            for order in (0, 1):
                want = ndimage.affine_transform(img, m[:, :2], m[:, 2], order=order, mode="nearest")
                assert want.tobytes() == warp_restated(img, m, order).tobytes(), (H, W, order)


def test_warp_checks_its_arguments_before_launching():
    from a_link_amd import augment
    table = np.zeros((2, 8, 8, 3), np.float32)
    eye = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (3, 1, 1))
    with pytest.raises(IndexError):
        augment.warp(table, [0, 2, 1], eye)
    with pytest.raises(ValueError):
        augment.warp(table, [0, 1, 1], eye, order=2)
    with pytest.raises(ValueError):
        augment.warp(table, None, eye)                       # three outputs, two images, no source rows
    with pytest.raises(ValueError):
        augment.warp(table, [0, 1], eye)
    assert augment.warp(table, [], np.zeros((0, 2, 3))).shape == (0, 8, 8, 3)


def test_warp_kernel_does_not_spill():
    """hipcc's resource report of csrc/augment.hip (written beside the object by the Makefile): no scratch in any kernel"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "augment.usage")
    text = open(path).read()
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert names and len(scratch) == len(names), path
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
