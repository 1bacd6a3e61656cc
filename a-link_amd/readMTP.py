"""readMTP — drop-in for the parts of reference code/readMTP.py the Multi-PIE driver calls:
qualifies / readAllImages (code/readMTP.py:8-39), resizeImages (:116-119), getGenerator (:80-113) and
createMiniBatch (:123-135).  Image files are read with PIL; resizing is the device bilinear kernel."""
import os

import numpy as np

from .alink_loop import createMiniBatchMTP as createMiniBatch  # noqa: F401
from .pairs import getGeneratorMTP as getGenerator, getNormalGenerator  # noqa: F401

_SUFFIXES = ("01_01_051_06.png", "02_01_051_06.png", "01_01_051_08.png", "02_01_051_08.png")


def qualifies(path):
    """the four (session, recording, camera 05_1, illumination 06/08) Multi-PIE shots the paper uses"""
    return path.endswith(_SUFFIXES)


def resizeImages(images, resize_res):
    from . import noise as _noise
    return [np.asarray(_noise.resize_images(images[0], resize_res)), np.asarray(_noise.resize_images(images[1], resize_res))]


def readAllImages(dirPath, resize=None):
    """-> list (one entry per person id = the file-name prefix before the first '_') of (k, H, W, C) arrays.  With `resize`
    = (width, height) the files are decoded first and then resized 1,024 at a time, each batch in one ragged launch
    (face_preprocess.preprocess_batch over the whole image): the pixels of noise.resize_images on every file, bit for bit."""
    from PIL import Image
    from . import face_preprocess
    person_wise = {}
    for path in os.listdir(dirPath):
        if qualifies(path):
            person_wise.setdefault(int(path.split('_')[0]), []).append(path)
    names = [(key, name) for key in person_wise for name in person_wise[key]]
    imgs = []
    for lo in range(0, len(names), 1024):
        batch = [np.asarray(Image.open(os.path.join(dirPath, name))) for _, name in names[lo:lo + 1024]]
        if resize:
            full = [(0, 0, a.shape[1], a.shape[0]) for a in batch]
            imgs.extend(face_preprocess.preprocess_batch(batch, bboxes=full, image_size=(resize[1], resize[0]), margin=0))
        else:
            imgs.extend(a.astype(np.float32) for a in batch)
    people, o = [], 0
    for key in person_wise:
        k = len(person_wise[key])
        people.append(np.stack(imgs[o:o + k]))
        o += k
    return people
