"""helpers — the helpers of reference code/helpers.py that the loop uses: roundoff (:39-46), one_hot (:32-36) and
augment_data (:114-141, the --augment switch of the drivers; the resampling runs on the GPU: augment.py)."""
import numpy as np


def roundoff(Y):
    y_ = []
    for y in Y:
        if y >= 0.5:
            y_.append([1])
        else:
            y_.append([0])
    return np.stack(y_)


def one_hot(Y, n_classes):
    """reference code/helpers.py:32-36"""
    y_ = np.zeros((len(Y), n_classes))
    y_[np.arange(len(Y)), Y] = 1
    return y_


def augment_data(dataset, dataset_labels, augementation_factor=1, use_random_rotation=True, use_random_shear=True,
                 use_random_shift=True, interpolation_order=1):
    """reference code/helpers.py:114-141 (the keyword's spelling is the reference's).  dataset = [left, right] pair images
    (n, H, W, C); per pair and round the result holds the original, then random_rotation(20), random_shear(0.2) and
    random_shift(0.2, 0.2) copies (each only when its use_* flag is on), left and right drawn independently from the global
    np.random stream in the reference's order; labels are repeated once per row.  Returns [left, right], labels.

    Same draws, same matrices and the same float32 pixels as keras_preprocessing 1.1 with scipy (augment.py).  Left and
    right must have the same H x W (the shift is drawn in pixels of it).  The images come back as float32, in the
    container they came in (NumPy, or CUDA tensors); interpolation_order = 0 gives the nearest-neighbour reading."""
    from . import augment
    left, right = dataset[0], dataset[1]
    if tuple(left.shape[1:3]) != tuple(right.shape[1:3]):
        raise ValueError("augment_data: left %s and right %s images differ in size" % (tuple(left.shape[1:3]), tuple(right.shape[1:3])))
    H, W = int(left.shape[1]), int(left.shape[2])
    plan = augment.draw(len(left), H, W, augementation_factor, use_random_rotation, use_random_shear, use_random_shift)
    out = [augment.warp(side, plan.src, plan.maps[s], interpolation_order, plan.copy[s]) for s, side in enumerate((left, right))]
    labels = dataset_labels.detach().cpu().numpy() if hasattr(dataset_labels, "detach") else np.asarray(dataset_labels)
    return out, labels[plan.src]
