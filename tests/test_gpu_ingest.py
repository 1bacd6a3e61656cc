"""GPU: the raw-photo front end through every layer — alink_ingest_faces (csrc/ingest.hip), face_preprocess, FaceModel.get_input,
ArcFace.process_raw, the readDFW loaders and ALINK_arc --face_boxes.

  * mode 0 (crop + resize) equals noise.resize_images (alink_resize_bilinear, the same device) on the cropped sub-array, bit
    for bit; mode 1 (warp) equals the NumPy float64 restatement of tests/ingest_ref.py — which tests/test_face_preprocess_host.py
    pins to scipy.ndimage.affine_transform(mode='grid-constant') — and scipy itself, bit for bit; one RAGGED table of photos of
    1 x 1 to 120 x 90 pixels per launch, outputs of 5 x 7 (one partly filled workgroup) and 112 x 112 (49 workgroups per photo),
    one and three channels, uint8 and float32 tables, both layouts;
  * a descriptor that does not fit the table yields a row of NaN and touches nothing else; bad scalars are ALINK_EINVAL;
  * the loaders equal a literal file-by-file loop, with and without face boxes."""
import os

import numpy as np
import pytest
import torch

from ingest_ref import random_similarity, warp_restatement, warp_scipy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """ArcFace holds a reference cycle (it binds its own process_screen), so the models built here — device memory, side and
    upload streams — outlive their tests until the cycle collector runs: run it when the module is done, before the next one"""
    yield
    import gc
    _MODE0_REF.clear()
    _MODE1_REF.clear()
    gc.collect()


SIZES = [(1, 1), (2, 3), (7, 5), (33, 17), (120, 90)]                # (H, W) of the photos of one table
OUTS = [(5, 7), (112, 112)]


def _photos(C, as_u8):
    rng = np.random.RandomState(100 + C)
    if as_u8:
        return [rng.randint(0, 256, (H, W, C)).astype(np.uint8) for H, W in SIZES]
    return [rng.uniform(0, 255, (H, W, C)).astype(np.float32) for H, W in SIZES]


def _ingest(photos, descs, Ho, Wo, layout="NHWC", table_elems=None, out=None, expect_rc=0, scalars=None):
    """alink_ingest_faces itself: descs = [(photo index, mode, box or None, m or None, overrides)] -> (n, Ho, Wo, C) NumPy"""
    from a_link_amd import _abi, face_preprocess as FP
    lib = _abi.init(0)
    as_u8 = photos[0].dtype == np.uint8
    C = photos[0].shape[2]
    table = np.concatenate([p.reshape(-1) for p in photos])
    offs = np.concatenate([[0], np.cumsum([p.size for p in photos])])
    d = np.zeros(len(descs), FP._DESC)
    for j, (i, mode, box, m, over) in enumerate(descs):
        d["offset"][j], d["H"][j], d["W"][j], d["mode"][j] = offs[i], photos[i].shape[0], photos[i].shape[1], mode
        if box is not None:
            d["box"][j] = box
        if m is not None:
            d["m"][j] = m
        for k, v in (over or {}).items():
            d[k][j] = v
    d_table = torch.from_numpy(table).cuda()
    d_desc = torch.from_numpy(d.view(np.uint8).reshape(-1)).cuda()
    n = len(descs)
    shape = (n, Ho, Wo, C) if layout == "NHWC" else (n, C, Ho, Wo)
    if out is None:
        out = torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
    args = dict(src_dtype=0 if as_u8 else 1, total=len(table) if table_elems is None else table_elems, n=n, C=C, Ho=Ho, Wo=Wo,
                layout=0 if layout == "NHWC" else 1)
    args.update(scalars or {})                                 # what the CALL is given; the buffers keep the sizes above
    rc = lib.alink_ingest_faces(_abi.ptr(d_table), args["src_dtype"], args["total"], _abi.ptr(d_desc), args["n"], args["C"],
                                args["Ho"], args["Wo"], args["layout"], _abi.ptr(out), _abi.current_stream(0))
    torch.cuda.synchronize()
    assert rc == expect_rc, (rc, lib.alink_last_error())
    got = out.cpu().numpy()
    return got if layout == "NHWC" else got.transpose(0, 2, 3, 1)


def _boxes(H, W):
    """the whole image, a 1-pixel-wide and a 1-pixel-high box, and boxes touching each edge"""
    out = [(0, 0, W, H), (W // 2, 0, W // 2 + 1, H), (0, H // 2, W, H // 2 + 1)]
    if H >= 7 and W >= 5:
        out += [(0, 1, W - 2, H - 1), (2, 1, W, H - 2), (1, 0, W - 1, H - 3), (1, 2, W - 2, H)]
    return out


_MODE0_REF = {}


def _mode0_reference(C, as_u8, Ho, Wo):
    """noise.resize_images on every cropped sub-array, one image per call; computed once per (C, dtype, size)"""
    from a_link_amd import noise
    key = (C, as_u8, Ho, Wo)
    if key not in _MODE0_REF:
        photos = _photos(C, as_u8)
        descs, want = [], []
        for i, p in enumerate(photos):
            for (x0, y0, x1, y1) in _boxes(*p.shape[:2]):
                descs.append((i, 0, (x0, y0, x1, y1), None, None))
                want.append(np.asarray(noise.resize_images(p[None, y0:y1, x0:x1].astype(np.float32), (Wo, Ho)))[0])
        _MODE0_REF[key] = (photos, descs, np.stack(want))
    return _MODE0_REF[key]


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("as_u8", [True, False])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_size", OUTS)
def test_crop_resize_equals_resize_images_on_the_crop(gpu, out_size, C, as_u8, layout):
    Ho, Wo = out_size
    photos, descs, want = _mode0_reference(C, as_u8, Ho, Wo)
    got = _ingest(photos, descs, Ho, Wo, layout)
    assert got.shape == want.shape and got.dtype == np.float32
    for j in range(len(descs)):
        assert got[j].tobytes() == want[j].tobytes(), (descs[j][:3], np.abs(got[j] - want[j]).max())


def _matrices(H, W, Ho, Wo, seed):
    rng = np.random.RandomState(seed)
    ms = [[1, 0, 0, 0, 1, 0],                                  # the identity
          [1, 0, -1, 0, 1, 0],                                 # sx = -1 at ox = 0 and sx = W at ox = W + 1, exactly
          [1, 0, 0, 0, 1, -1],                                 # the same along y
          [1, 0, W, 0, 1, 0], [1, 0, 0, 0, 1, -float(Ho)],     # sx = W at ox = 0; sy <= -1 everywhere: all zeros
          [1, 0, -0.5, 0, 1, H - 0.75],                        # partly outside: the border blends with black
          [0.5, 0, -0.75, 0, 0.5, -0.25]]
    return ms + [random_similarity(rng, H, W, Ho, Wo) for _ in range(4)]


_MODE1_REF = {}


def _mode1_reference(C, as_u8, Ho, Wo):
    key = (C, as_u8, Ho, Wo)
    if key not in _MODE1_REF:
        photos = _photos(C, as_u8)
        descs, want = [], []
        for i, p in enumerate(photos):
            for m in _matrices(p.shape[0], p.shape[1], Ho, Wo, 7 * i + C):
                descs.append((i, 1, None, m, None))
                want.append(warp_restatement(p, m, Ho, Wo))
        _MODE1_REF[key] = (photos, descs, np.stack(want))
    return _MODE1_REF[key]


@pytest.mark.parametrize("layout", ["NHWC", "NCHW"])
@pytest.mark.parametrize("as_u8", [True, False])
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("out_size", OUTS)
def test_warp_equals_restatement_and_scipy(gpu, out_size, C, as_u8, layout):
    Ho, Wo = out_size
    photos, descs, want = _mode1_reference(C, as_u8, Ho, Wo)
    got = _ingest(photos, descs, Ho, Wo, layout)
    for j, (i, _, _, m, _) in enumerate(descs):
        assert got[j].tobytes() == want[j].tobytes(), (SIZES[i], m, np.abs(got[j] - want[j]).max())
    per = len(descs) // len(photos)
    for i, p in enumerate(photos):
        H, W = p.shape[:2]
        ident = got[i * per]                                    # the identity: the source's top-left window, zeros beyond it
        h, w = min(H, Ho), min(W, Wo)
        assert np.array_equal(ident[:h, :w], p[:h, :w].astype(np.float32)) and not ident[h:].any() and not ident[:, w:].any()
        shift = got[i * per + 1]                                # sx = ox - 1: column 0 (sx = -1) and column W + 1 (sx = W) are 0
        assert not shift[:, 0].any() and not shift[:, W + 1:].any()
        assert np.array_equal(shift[:h, 1:min(W, Wo - 1) + 1], p[:h, :min(W, Wo - 1)].astype(np.float32))
        assert not got[i * per + 3].any() and not got[i * per + 4].any()
        assert got[i * per + 5].any()
    if layout == "NHWC":                                        # scipy itself, once per (C, dtype, size)
        for j, (i, _, _, m, _) in enumerate(descs):
            assert got[j].tobytes() == warp_scipy(photos[i], m, Ho, Wo).tobytes(), (SIZES[i], m)


@pytest.mark.parametrize("as_u8", [True, False])
def test_mixed_modes_in_one_launch(gpu, as_u8):
    Ho, Wo = 112, 112
    photos, d0, want0 = _mode0_reference(3, as_u8, Ho, Wo)
    _, d1, want1 = _mode1_reference(3, as_u8, Ho, Wo)
    order = [(0, j) for j in range(len(d0))] + [(1, j) for j in range(len(d1))]
    np.random.RandomState(1).shuffle(order)
    got = _ingest(photos, [(d0, d1)[k][j] for k, j in order], Ho, Wo)
    for g, (k, j) in zip(got, order):
        assert g.tobytes() == (want0, want1)[k][j].tobytes(), (k, j)


def test_bad_descriptor_yields_nan_row_and_neighbours_are_untouched(gpu):
    photos, d0, want0 = _mode0_reference(3, True, 5, 7)
    _, d1, want1 = _mode1_reference(3, True, 5, 7)
    total = sum(p.size for p in photos)
    good0, good1 = d0[-1], d1[-1]                              # the 120 x 90 photo: the last one of the table
    bad = [(4, 0, (0, 0, 90, 120), None, {"offset": total}),                 # an offset past the table
           (4, 0, (0, 0, 90, 120), None, {"offset": total - 120 * 90 * 3 + 1}),   # the photo's last element past it
           (4, 1, None, [1, 0, 0, 0, 1, 0], {"offset": -1}),
           (4, 0, (5, 5, 5, 9), None, None), (4, 0, (5, 9, 8, 9), None, None),    # empty boxes
           (4, 0, (0, 0, 91, 120), None, None), (4, 0, (-1, 0, 90, 120), None, None),     # boxes that leave the image
           (4, 1, None, [1, 0, 0, 0, 1, 0], {"H": 0}), (4, 1, None, [1, 0, 0, 0, 1, 0], {"W": -3}),
           (4, 1, None, [1, 0, 0, 0, 1, 0], {"H": 2 ** 31 - 1, "W": 2 ** 31 - 1}),  # 2^62 pixels: no product in the check may wrap
           (4, 7, (0, 0, 90, 120), [1, 0, 0, 0, 1, 0], None)]                     # an unknown mode
    descs = []
    for b in bad:
        descs += [good0, b, good1]
    for layout in ("NHWC", "NCHW"):
        got = _ingest(photos, descs, 5, 7, layout)
        for k in range(len(bad)):
            assert got[3 * k].tobytes() == want0[-1].tobytes() and got[3 * k + 2].tobytes() == want1[-1].tobytes(), k
            assert np.isnan(got[3 * k + 1]).all(), (k, bad[k])
    # a table shorter than the descriptors say: every photo that does not fit it is NaN, the ones that do are computed
    short = _ingest(photos, d0, 5, 7, table_elems=total - 1)
    last = [j for j, d in enumerate(d0) if d[0] == 4]
    assert np.isnan(short[last]).all()
    assert short[:last[0]].tobytes() == want0[:last[0]].tobytes()


def test_bad_scalars_are_einval(gpu):
    from a_link_amd import _abi
    photos, d0, _ = _mode0_reference(3, False, 5, 7)
    for scalars in (dict(C=0), dict(Ho=0), dict(Wo=-1), dict(layout=2), dict(src_dtype=2), dict(n=-1), dict(total=-1)):
        got = _ingest(photos, d0[:2], 5, 7, expect_rc=-1, scalars=scalars)
        assert (got == -7.0).all(), scalars                      # nothing was launched
    # 49 workgroups per photo: 43,826,197 photos would be 2^31 + 5 of them
    assert (_ingest(photos, d0[:2], 112, 112, expect_rc=-1, scalars=dict(n=43826197)) == -7.0).all()
    assert _abi.load().alink_last_error()
    # dev_out inside the table
    from a_link_amd import face_preprocess as FP
    lib = _abi.init(0)
    table = torch.zeros(4096, dtype=torch.float32, device="cuda")
    d = np.zeros(1, FP._DESC)
    d["H"], d["W"], d["box"] = 4, 4, (0, 0, 4, 4)
    d_desc = torch.from_numpy(d.view(np.uint8).reshape(-1)).cuda()
    for out in (table, table[4000:]):
        rc = lib.alink_ingest_faces(_abi.ptr(table), 1, 4096, _abi.ptr(d_desc), 1, 3, 5, 7, 0, _abi.ptr(out), _abi.current_stream(0))
        assert rc == -1 and b"overlap" in lib.alink_last_error()
    assert _ingest(photos, [], 5, 7).shape == (0, 5, 7, 3)       # n = 0: nothing to do, no error


def test_preprocess_batch_raises_before_any_launch(gpu, monkeypatch):
    from a_link_amd import _abi, face_preprocess as FP
    photos = _photos(3, True)

    def no_launch(*a, **k):
        raise AssertionError("reached the device")
    monkeypatch.setattr(_abi, "init", no_launch)
    n = len(photos)
    for kw in (dict(bboxes=[None] * 4 + [(5, 5, 5, 9)], margin=0),                 # an empty box
               dict(bboxes=[None] * 4 + [(200, 0, 260, 50)], margin=0),            # a box outside its photo
               dict(bboxes=[(0, 0, 1, 1)] * (n - 1)),                              # one box too few
               dict(landmarks=[None] * 4 + [np.zeros((5, 2))]),                    # degenerate landmarks
               dict(landmarks=[None] * 4 + [np.full((5, 2), np.nan)]),
               dict(layout="CHWN"), dict(image_size=(0, 112))):
        with pytest.raises(ValueError):
            FP.preprocess_batch(photos, **kw)
    with pytest.raises(ValueError):
        FP.preprocess_batch(photos + [np.zeros((4, 4), np.uint8)])
    with pytest.raises(ValueError):
        FP.preprocess_batch(photos + [np.zeros((4, 4, 1), np.uint8)])


def test_preprocess_batch_routes_and_chunks(gpu, monkeypatch):
    """the three routes per photo in one call, against the raw kernel; float32 as soon as one photo is; a table limit that
    cuts the batch into several launches changes nothing"""
    from a_link_amd import face_preprocess as FP, noise
    photos = _photos(3, True)[2:] + [np.random.RandomState(0).uniform(0, 255, (60, 50, 3)).astype(np.float32)]
    lm = FP.template() * 0.7 + [10, 20]
    got = FP.preprocess_batch(photos, bboxes=[None, (3, 4, 12, 20), (10, 10, 60, 80), None], landmarks=[None, None, None, lm],
                              margin=6)
    assert isinstance(got, np.ndarray) and got.shape == (4, 112, 112, 3) and got.dtype == np.float32

    def crop(p, box):
        x0, y0, x1, y1 = box
        return np.asarray(noise.resize_images(p[None, y0:y1, x0:x1].astype(np.float32), (112, 112)))[0]
    assert got[0].tobytes() == crop(photos[0], (0, 0, 5, 7)).tobytes()                 # centre crop of 7 x 5: int(0.3125) = 0
    assert got[1].tobytes() == crop(photos[1], (0, 1, 15, 23)).tobytes()
    assert got[2].tobytes() == crop(photos[2], (7, 7, 63, 83)).tobytes()
    m = FP.invert_affine(FP.estimate_similarity(lm))[0].reshape(-1)
    assert got[3].tobytes() == warp_restatement(photos[3], m, 112, 112).tobytes()
    monkeypatch.setattr(FP, "TABLE_BYTES", 4 * 33 * 17 * 3 + 8)                          # float32 table: at most one big photo each
    again = FP.preprocess_batch(photos, bboxes=[None, (3, 4, 12, 20), (10, 10, 60, 80), None], landmarks=[None, None, None, lm],
                                margin=6)
    assert again.tobytes() == got.tobytes()
    dev = FP.preprocess_batch([torch.from_numpy(p) for p in photos[:2]], layout="NCHW", image_size=(5, 7))
    assert dev.is_cuda and tuple(dev.shape) == (2, 3, 5, 7)
    assert np.array_equal(dev.cpu().numpy().transpose(0, 2, 3, 1), FP.preprocess_batch(photos[:2], image_size="5,7"))
    assert FP.preprocess_batch([]).shape == (0, 112, 112, 3)


def test_round_trip_through_landmarks(gpu):
    """a 112 x 112 face pasted at an integer offset into a black canvas, its landmarks the template plus that offset: the
    estimate is the shift to ~1e-13, so only the float32 rounding of values <= 255 remains — 1e-4 grey levels"""
    from a_link_amd import face_preprocess as FP
    rng = np.random.RandomState(9)
    faces, canvases, marks = [], [], []
    for (H, W, oy, ox), as_u8 in zip(((300, 260, 37, 101), (150, 170, 0, 58), (112, 112, 0, 0)), (True, False, True)):
        face = rng.randint(0, 256, (112, 112, 3)).astype(np.uint8) if as_u8 else rng.uniform(0, 255, (112, 112, 3)).astype(np.float32)
        canvas = np.zeros((H, W, 3), face.dtype)
        canvas[oy:oy + 112, ox:ox + 112] = face
        faces.append(face.astype(np.float32))
        canvases.append(canvas)
        marks.append(FP.template() + [ox, oy])
    got = FP.preprocess_batch(canvases[:1] + canvases[2:], landmarks=marks[:1] + marks[2:])      # a uint8 table
    assert np.abs(got[0] - faces[0]).max() < 1e-4 and np.abs(got[1] - faces[2]).max() < 1e-4
    got = FP.preprocess_batch(canvases, landmarks=marks)                                          # a float32 one
    for g, f in zip(got, faces):
        assert np.abs(g - f).max() < 1e-4, np.abs(g - f).max()
    one = FP.preprocess(canvases[0], landmark=marks[0], image_size='112,112')
    assert one.shape == (112, 112, 3) and one.tobytes() == got[0].tobytes()


def test_get_input_and_process_raw(gpu):
    from a_link_amd import face_model, face_preprocess as FP, siamese
    fm = face_model.FaceModel(siamese._Args({"image_size": "112,112", "model": "", "threshold": 1.24}))
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, (140, 130, 3)).astype(np.uint8)
    assert np.array_equal(fm.get_input(img), np.transpose(img, (2, 0, 1)))                        # as it has always been
    lm = FP.template() * 0.9 + [12, 9]
    box = (20, 30, 100, 120)
    assert fm.get_input(img, landmark=lm).tobytes() == np.transpose(FP.preprocess(img, None, lm, image_size='112,112'), (2, 0, 1)).tobytes()
    assert fm.get_input(img, bbox=box).tobytes() == np.transpose(FP.preprocess(img, box, image_size='112,112'), (2, 0, 1)).tobytes()
    assert fm.get_input(img, box, lm).shape == (3, 112, 112)

    size = (32, 32)
    conv = siamese.ArcFace(size, "synthetic:r18:3")
    photos = [rng.randint(0, 256, (rng.randint(30, 80), rng.randint(30, 80), 3)).astype(np.uint8) for _ in range(7)]
    marks = [FP.template(size) * rng.uniform(0.5, 1.5) + rng.uniform(0, 10, 2) if i % 2 else None for i in range(7)]
    boxes = [None, None, (5, 5, 25, 28), None, None, None, (0, 0, 30, 30)]
    # process_raw walks the photos max_batch at a time: 3 makes it three chunks of the 7.  Only for that call — the reference
    # below is ONE launch chain, and neither side takes a stream from torch's pool (a model built with max_batch=3 would take
    # three for its multi-chunk form, and which pool stream a LATER model gets decides how its streams share hardware queues)
    bb = conv.model.model
    full, bb.max_batch = bb.max_batch, 3
    try:
        got = conv.process_raw(photos, landmarks=marks, bboxes=boxes)
    finally:
        bb.max_batch = full
    want = conv.process(FP.preprocess_batch(photos, bboxes=boxes, landmarks=marks, image_size=size))
    assert isinstance(got, np.ndarray) and got.shape == (7, 512) and got.tobytes() == np.asarray(want).tobytes()
    assert conv.process_raw([]).shape == (0, 512)


# ---- the loaders -------------------------------------------------------------------------------------------------------
def _literal_people(root, imageRes, faceBoxes=None):
    """the loaders' one-file-at-a-time form: PIL (-> crop) -> float32 -> noise.resize_images, per person and kind"""
    from PIL import Image
    from a_link_amd import noise
    d = os.path.join(root, "Training_data")
    for person in sorted(os.listdir(d)):
        kinds = {"plain": [], "dig": [], "imp": []}
        for name in sorted(os.listdir(os.path.join(d, person))):
            img = Image.open(os.path.join(d, person, name)).convert('RGB')
            if faceBoxes is not None:
                img = img.crop(faceBoxes[os.path.join("Training_data", person, name)])
            img = np.asarray(noise.resize_images(np.asarray(img, dtype=np.float32)[None], imageRes))[0]
            stem = name.rsplit('.', 1)[0]
            kinds["dig" if '_h_' in stem else ("imp" if '_I_' in stem else "plain")].append(img)
        yield kinds


def _face_boxes(root):
    """a fractional box inside every photo of the synthetic tree (the smallest is 50 x 50), one of them the whole photo"""
    from PIL import Image
    rng = np.random.RandomState(3)
    boxes = {}
    d = os.path.join(root, "Training_data")
    for person in sorted(os.listdir(d)):
        for name in sorted(os.listdir(os.path.join(d, person))):
            W, H = Image.open(os.path.join(d, person, name)).size
            l, u = rng.uniform(0, W / 3.0), rng.uniform(0, H / 3.0)
            boxes[os.path.join("Training_data", person, name)] = [l, u, rng.uniform(l + 20, W), rng.uniform(u + 20, H)]
    first = sorted(boxes)[0]
    W, H = Image.open(os.path.join(root, first)).size
    boxes[first] = [0, 0, W, H]
    return boxes


@pytest.mark.parametrize("with_boxes", [False, True])
def test_dfw_loaders_equal_a_file_by_file_loop(gpu, tmp_path, with_boxes):
    from a_link_amd import readDFW, siamese
    from test_gpu_driver import _make_dfw
    root = _make_dfw(str(tmp_path))
    boxes = _face_boxes(root) if with_boxes else None
    kw = dict(faceBoxes=boxes) if with_boxes else {}
    res = (112, 112)
    people = list(_literal_people(root, res, boxes))
    want_plain = [np.stack(k["plain"]) for k in people if k["dig"] and k["imp"]]
    want_dig = [np.stack(k["dig"]) for k in people if k["dig"] and k["imp"]]
    Rp, Rd = readDFW.getRawTrainData(root, "Training_data", res, **kw)
    assert len(Rp) == len(want_plain) == 6 and len(Rd) == 6
    for a, b in zip(Rp + Rd, want_plain + want_dig):
        assert a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
    conv = siamese.ArcFace(res, "synthetic:r18:2")
    Xp, Xd, Xi = readDFW.getAllTrainData(root, "Training_data", res, conv, **kw)
    kept = [k for k in people if k["dig"] and k["imp"] and k["plain"]]
    assert len(Xp) == len(Xd) == len(Xi) == len(kept) == 6
    for got, kind in ((Xp, "plain"), (Xd, "dig"), (Xi, "imp")):
        for g, k in zip(got, kept):
            assert np.array_equal(g, conv.process(np.stack(k[kind])))
    if with_boxes:                                               # a photo without a box is skipped; so is a box that misses its photo
        fewer = dict(boxes)
        del fewer["Training_data/person00/00_a.png"]
        fewer["Training_data/person01/01_a.png"] = [500, 500, 600, 600]
        Rp2, Rd2 = readDFW.getRawTrainData(root, "Training_data", res, faceBoxes=fewer)
        assert [len(p) for p in Rp2] == [1, 1, 2, 2, 2, 2] and Rp2[0].tobytes() == Rp[0][:1].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(Rd2, Rd))


def test_mtp_loader_equals_a_file_by_file_loop(gpu, tmp_path):
    from PIL import Image
    from a_link_amd import noise, readMTP
    rng = np.random.RandomState(6)
    names = ["%03d_%s" % (p, s) for p in (1, 2) for s in readMTP._SUFFIXES[:2 + p]]
    for k, name in enumerate(names):
        Image.fromarray(rng.randint(0, 256, (40 + 3 * k, 50 - 2 * k, 3)).astype(np.uint8)).save(str(tmp_path / name))
    got = readMTP.readAllImages(str(tmp_path), (32, 24))
    assert sorted(len(p) for p in got) == [3, 4] and got[0].shape[1:] == (24, 32, 3) and got[0].dtype == np.float32
    want = {}
    for name in os.listdir(str(tmp_path)):
        img = np.asarray(Image.open(str(tmp_path / name)), dtype=np.float32)
        want.setdefault(int(name.split('_')[0]), []).append(np.asarray(noise.resize_images(img[None], (32, 24)))[0])
    for g, key in zip(got, want):
        assert g.tobytes() == np.stack(want[key]).tobytes()


def test_driver_runs_with_face_boxes(gpu, tmp_path):
    """ALINK_arc.main(... --face_boxes FILE) end to end: both phases on the synthetic DFW tree, cropped at load"""
    from a_link_amd import ALINK_arc
    from test_gpu_driver import _make_dfw
    root = _make_dfw(str(tmp_path))
    coords = str(tmp_path / "Training_data_face_coordinate.txt")
    with open(coords, "w") as f:
        for name, box in sorted(_face_boxes(root).items()):
            f.write("%s %s\n" % (name, " ".join(repr(float(v)) for v in box)))
    models = str(tmp_path / "models")
    os.makedirs(models)
    common = ["--dataDirPrefix", root, "--arcface_model", "synthetic:r18:2", "--quiet", "--face_boxes", coords,
              "--out_model", os.path.join(models, "postALINK"), "--ensemble_basepath", os.path.join(models, "ensemble"),
              "--disguised_basemodel", os.path.join(models, "disguisedModel"), "--pretrain_steps", "64",
              "--dig_epochs", "1", "--undig_epochs", "1", "--noise", "gaussian,speckle"]
    np.random.seed(0)
    assert ALINK_arc.main(common + ["--train_disguised_model"]) is None
    st = ALINK_arc.main(common + ["--alink_bs", "3", "--batch_send", "2", "--disparity_ratio", "1.0", "--eps", "0.0",
                                  "--ft_epochs", "1", "--active_ratio", "4.0"])
    assert os.path.exists(os.path.join(models, "postALINK.h5"))
    assert st.iterations >= 1
    assert ALINK_arc.build_parser().parse_args([]).face_boxes is None
