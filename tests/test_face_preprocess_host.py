"""CPU: the host half of the raw-photo front end (a-link_amd/face_preprocess.py, readDFW.constructIndexMap) and the rule the
GPU half is held to.

  * the NumPy restatement of alink_ingest_faces' warp (tests/ingest_ref.py) equals scipy.ndimage.affine_transform(order=1,
    mode='grid-constant') bit for bit: tests/test_gpu_ingest.py compares the kernel with that restatement;
  * estimate_similarity (Umeyama, SVD) against an independently written closed form for two dimensions;
  * invert_affine, constructIndexMap, and the margin / centre-crop box arithmetic on hand-computed cases."""
import numpy as np
import pytest

import a_link_amd  # noqa: F401
from a_link_amd import face_preprocess as FP, readDFW

from ingest_ref import closed_form_similarity, random_similarity, warp_restatement, warp_scipy


def test_restatement_equals_scipy_grid_constant():
    rng = np.random.RandomState(11)
    for case in range(24):
        H, W = rng.randint(40, 121, 2)
        Ho, Wo = ((112, 112), (5, 7), (40, 56))[case % 3]
        img = rng.randint(0, 256, (H, W, 3)).astype(np.uint8) if case % 2 else rng.uniform(0, 255, (H, W, 3)).astype(np.float32)
        m = random_similarity(rng, H, W, Ho, Wo)
        got, want = warp_restatement(img, m, Ho, Wo), warp_scipy(img, m, Ho, Wo)
        assert got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes(), (case, np.abs(got - want).max())
    # the coordinates the rule's edges sit on: sx = -1 and sx = W exactly (both 0), a source wholly outside, the identity
    img = rng.randint(0, 256, (6, 5, 2)).astype(np.uint8)
    for m in ([1, 0, -1, 0, 1, 0], [1, 0, 0, 0, 1, -1], [1, 0, 40, 0, 1, 0], [1, 0, 0, 0, 1, 0], [1, 0, -0.5, 0, 1, -0.25]):
        got, want = warp_restatement(img, m, 9, 8), warp_scipy(img, m, 9, 8)
        assert got.tobytes() == want.tobytes(), m
    assert not warp_restatement(img, [1, 0, 40, 0, 1, 0], 9, 8).any()
    ident = warp_restatement(img, [1, 0, 0, 0, 1, 0], 9, 8)
    assert np.array_equal(ident[:6, :5], img.astype(np.float32)) and not ident[6:].any() and not ident[:, 5:].any()


def _posed_template(rng, image_size=(112, 112)):
    t = FP.template(image_size)
    th, s = rng.uniform(-np.pi, np.pi), rng.uniform(0.3, 3.0)
    R = s * np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return t @ R.T + rng.uniform(0, 60, 2)


def test_umeyama_equals_closed_form():
    """1e-9 absolute: the two forms differ by ~1e-13 at coordinates of a few hundred pixels, and the error grows with the
    coordinates' size — the bound leaves room for photos of several thousand pixels"""
    rng = np.random.RandomState(5)
    for size in ((112, 112), (112, 96)):
        lm = np.stack([_posed_template(rng, size) + rng.normal(0, 1.5, (5, 2)) for _ in range(50)])
        assert np.abs(lm).max() < 400
        got = FP.estimate_similarity(lm, size)
        assert got.shape == (50, 2, 3) and got.dtype == np.float64
        for i in range(50):
            want = closed_form_similarity(lm[i], FP.template(size))
            assert np.abs(got[i] - want).max() < 1e-9, (i, np.abs(got[i] - want).max())
        assert np.array_equal(FP.estimate_similarity(lm[3], size)[0], got[3])           # one face, (5, 2)


def test_template_and_exact_landmarks():
    assert FP.ARCFACE_TEMPLATE.shape == (5, 2)
    assert np.abs(FP.template((112, 112)) - (FP.ARCFACE_TEMPLATE + [8, 0])).max() < 1e-5          # float32 roundings only
    assert np.abs(FP.template((112, 96)) - FP.ARCFACE_TEMPLATE).max() < 1e-5
    for size in ((112, 112), (112, 96), "112,112"):
        M = FP.estimate_similarity(FP.template(size), size)[0]
        assert np.abs(M - np.array([[1.0, 0, 0], [0, 1.0, 0]])).max() < 1e-9
    shifted = FP.estimate_similarity(FP.template() + [37, 11])[0]
    assert np.abs(shifted - np.array([[1.0, 0, -37], [0, 1.0, -11]])).max() < 1e-9


def test_mirrored_landmarks_give_a_rotation():
    rng = np.random.RandomState(2)
    lm = _posed_template(rng)
    lm[:, 0] = 200.0 - lm[:, 0]                                    # a mirror image: no rotation maps it onto the template
    M = FP.estimate_similarity(lm)[0]
    assert np.linalg.det(M[:, :2]) > 0
    assert abs(M[0, 0] - M[1, 1]) < 1e-9 and abs(M[0, 1] + M[1, 0]) < 1e-9
    assert np.abs(M - closed_form_similarity(lm, FP.template())).max() < 1e-9


def test_degenerate_landmarks_raise():
    for bad in (np.zeros((5, 2)), np.full((5, 2), 17.25), np.full((5, 2), np.nan), np.zeros((5, 3)), np.zeros((4, 2))):
        with pytest.raises(ValueError):
            FP.estimate_similarity(bad)
    nan_one = FP.template().copy()
    nan_one[2, 1] = np.inf
    with pytest.raises(ValueError):
        FP.estimate_similarity(np.stack([FP.template(), nan_one]))


def test_invert_affine():
    rng = np.random.RandomState(8)
    lm = np.stack([_posed_template(rng) for _ in range(20)])
    M = FP.estimate_similarity(lm)
    inv = FP.invert_affine(M)
    assert inv.shape == (20, 2, 3)
    for a, b in zip(M, inv):
        prod = np.vstack([a, [0, 0, 1]]) @ np.vstack([b, [0, 0, 1]])
        assert np.abs(prod - np.eye(3)).max() < 1e-12
    # hand-computed: x' = 2x + 3, y' = 4y - 8  <->  x = x'/2 - 1.5, y = y'/4 + 2
    assert np.array_equal(FP.invert_affine([[2.0, 0, 3], [0, 4.0, -8]]), [[0.5, 0, -1.5], [0, 0.25, 2.0]])
    assert np.array_equal(FP.invert_affine([[1.0, 2, 5], [2.0, 4, 7]]), np.zeros((2, 3)))       # singular: D = 0 stays 0


def test_construct_index_map(tmp_path):
    path = tmp_path / "coords.txt"
    path.write_text("Training_data/Ann Lee/Ann Lee_h_001.jpg 10 20.5 110 140\n"
                    "Training_data/Bo/Bo.jpg 0 0 64 64   \n"
                    "\n"
                    "Training_data/Bo/Bo_I_001.jpg 3.25 4 5 6\n")
    m = readDFW.constructIndexMap(str(path))
    assert m == {"Training_data/Ann Lee/Ann Lee_h_001.jpg": [10.0, 20.5, 110.0, 140.0],
                 "Training_data/Bo/Bo.jpg": [0.0, 0.0, 64.0, 64.0],
                 "Training_data/Bo/Bo_I_001.jpg": [3.25, 4.0, 5.0, 6.0]}


def test_margin_and_centre_crop_rule():
    # a box in the middle: 22 pixels more on every side
    assert FP.crop_box((200, 300, 3), (100, 50, 180, 150)) == (78, 28, 202, 172)
    # at the top-left corner the margin is cut off at 0, at the bottom-right one at the photo's size
    assert FP.crop_box((200, 300, 3), (0, 0, 50, 60)) == (0, 0, 72, 82)
    assert FP.crop_box((200, 300, 3), (250, 150, 300, 200)) == (228, 128, 300, 200)
    assert FP.crop_box((200, 300, 3), (10, 5, 295, 190), margin=45) == (0, 0, 300, 200)          # 45 // 2 = 22
    # fractions are truncated after the margin, as an int32 assignment does
    assert FP.crop_box((200, 300, 3), (100.7, 50.2, 180.9, 150.5), margin=10) == (95, 45, 185, 155)
    assert FP.crop_box((200, 300, 3), (100, 50, 180, 150), margin=0) == (100, 50, 180, 150)
    # no box: int(6.25 %) off every side, then the margin — 300 x 200: (18, 12, 282, 188) widened by 22 and clipped
    assert FP.crop_box((200, 300, 3)) == (0, 0, 300, 200)
    assert FP.crop_box((200, 300, 3), margin=0) == (18, 12, 282, 188)
    assert FP.crop_box((1000, 800), margin=44) == (28, 40, 772, 960)
    assert FP.crop_box((10, 10, 3), margin=0) == (0, 0, 10, 10)                                  # int(0.625) = 0
    for bad in ((50, 50, 10, 10), (400, 0, 500, 100), (0, 0, np.nan, 5), (1, 2, 3)):
        with pytest.raises(ValueError):
            FP.crop_box((200, 300, 3), bad, margin=0)


def test_pil_box_rounds_like_image_crop_and_clips():
    from PIL import Image
    img = Image.fromarray(np.arange(20 * 30 * 3, dtype=np.uint8).reshape(20, 30, 3))
    for box in ((2.5, 3.5, 11.49, 17.51), (0.4, 0, 29.6, 20), (4, 5, 6, 7)):
        x0, y0, x1, y1 = readDFW._pil_box(box, 20, 30)
        assert np.array_equal(np.asarray(img.crop(box)), np.asarray(img)[y0:y1, x0:x1]), box
    assert readDFW._pil_box((-5.2, -1, 40, 12.2), 20, 30) == (0, 0, 30, 12)                       # PIL would pad with black
    assert readDFW._pil_box((31, 0, 40, 10), 20, 30) is None and readDFW._pil_box((5, 5, 5, 9), 20, 30) is None
