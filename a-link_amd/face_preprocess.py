"""face_preprocess — the raw-photo front end of reference code/face_preprocess.py:46-111, batched on the GPU.

    ARCFACE_TEMPLATE / template(image_size)        the five points of code/face_preprocess.py:61-68
    estimate_similarity(landmarks, image_size)     skimage's SimilarityTransform.estimate (:71-73): Umeyama's least squares
    invert_affine(M)                               what cv2.warpAffine does to M before it samples
    crop_box(shape, bbox, margin)                  the margin / centre-crop rule (:76-91)
    preprocess_batch(images, bboxes, landmarks)    any number of photos, each of its own size, in ONE launch
    preprocess(img, bbox, landmark, **kwargs)      the reference's signature, one image

Per photo one of three routes, as in the reference: five landmarks give a similarity warp onto the ArcFace template; otherwise
a face box is widened by margin // 2 on every side, clipped to the photo, cropped and resized; otherwise the photo's central
87.5 % (6.25 % off every side) is taken for the box.  The pixels are computed by alink_ingest_faces (csrc/ingest.hip): the
batch is packed into one pinned table (uint8 when every photo is uint8, else float32), uploaded once and resampled by one
launch, whatever the photos' sizes.  The five-point estimate is a few dozen float64 flops per face and stays on the host.

Differences from the reference, all deliberate:
  * the result is unrounded float32 0..255, as everywhere upstream of the models; cv2 on uint8 photos rounds to uint8;
  * the warp interpolates at exact float64 coordinates with a black border (scipy.ndimage.affine_transform's order-1
    'grid-constant' rule, bit for bit); cv2.warpAffine quantises coordinates to 1/32 pixel and weights to 15 bits.  cv2 is not a
    dependency and no equality with it is claimed;
  * the crop + resize is alink_resize_bilinear's rule (cv2.resize INTER_LINEAR on float32) relative to the box;
  * landmarks are used in float64; the reference casts them to float32 first (:69).  The template is the reference's float32
    numbers (the + 8 included), widened;
  * an invalid box (empty after clipping, not finite) raises ValueError; the reference hands cv2 an empty array.
No face detector is provided: boxes and landmarks come from the caller.
"""
import ctypes as C

import numpy as np

from . import _abi

# (x, y) of left eye, right eye, nose tip, left and right mouth corner in a 96-wide, 112-high aligned face
ARCFACE_TEMPLATE = np.array([[30.2946, 51.6963],
                             [65.5318, 51.5014],
                             [48.0252, 71.7366],
                             [33.5493, 92.3655],
                             [62.7299, 92.2041]], dtype=np.float64)

TABLE_BYTES = 256 << 20          # a chunk's packed table stays under this (one photo alone may exceed it)

_DESC = np.dtype([("offset", np.int64), ("H", np.int32), ("W", np.int32), ("mode", np.int32), ("box", np.int32, 4),
                  ("m", np.float64, 6)], align=True)
assert _DESC.itemsize == C.sizeof(_abi.IngestDesc) and _DESC.fields["m"][1] == _abi.IngestDesc.m.offset


def _size(image_size):
    """(height, width) from the reference's forms: '112,112', '112', (112, 112)"""
    if isinstance(image_size, str):
        image_size = [int(x) for x in image_size.split(',')]
    image_size = [int(v) for v in np.atleast_1d(image_size)]
    if len(image_size) == 1:
        image_size = [image_size[0], image_size[0]]
    if len(image_size) != 2 or min(image_size) < 1:
        raise ValueError("image_size must be (height, width), got %r" % (image_size,))
    return image_size[0], image_size[1]


def template(image_size=(112, 112)):
    """The (5, 2) float64 template for faces of image_size = (height, width): x shifted by 8 when the width is 112, with the
    reference's float32 roundings (code/face_preprocess.py:61-68)."""
    src = ARCFACE_TEMPLATE.astype(np.float32)
    if _size(image_size)[1] == 112:
        src[:, 0] += 8.0
    return src.astype(np.float64)


def estimate_similarity(landmarks, image_size=(112, 112)):
    """Least-squares similarity (rotation, uniform scale, shift; no reflection) taking each face's five landmarks onto the
    template: (n, 5, 2) or (5, 2) (x, y) points -> (n, 2, 3) float64, dst = M[:, :2] . src + M[:, 2].
    Umeyama (1991), the SVD form: with demeaned points and A = dst^T src / 5 = U S V^T, R = U diag(1, sign det A) V^T,
    scale = (S . diag) / var(src), t = mean(dst) - scale R mean(src).  Raises ValueError for degenerate landmarks."""
    src = np.asarray(landmarks, dtype=np.float64)
    if src.ndim == 2:
        src = src[None]
    if src.ndim != 3 or src.shape[1:] != (5, 2):
        raise ValueError("landmarks must be (n, 5, 2) points, got %s" % (src.shape,))
    dst = template(image_size)
    n = len(src)
    if n == 0:
        return np.zeros((0, 2, 3))
    if not np.isfinite(src).all():
        raise ValueError("landmarks are not finite")
    src_mean, dst_mean = src.mean(axis=1), dst.mean(axis=0)
    sd, dd = src - src_mean[:, None, :], dst - dst_mean
    var = (sd ** 2).sum(axis=(1, 2)) / 5.0
    if (var <= 0).any():
        raise ValueError("degenerate landmarks: the five points of face %d coincide" % int(np.argmax(var <= 0)))
    A = np.einsum("ki,nkj->nij", dd, sd) / 5.0                      # (n, 2, 2)
    U, S, Vt = np.linalg.svd(A)
    sign = np.where(np.linalg.det(A) < 0, -1.0, 1.0)
    # collinear landmarks (rank 1): det A is 0 up to rounding, and the sign that keeps R a rotation is that of det U det V
    rank1 = S[:, 1] <= S[:, 0] * 2 * np.finfo(np.float64).eps
    sign = np.where(rank1, np.where(np.linalg.det(U) * np.linalg.det(Vt) < 0, -1.0, 1.0), sign)
    D = np.zeros((n, 2, 2))
    D[:, 0, 0], D[:, 1, 1] = 1.0, sign
    R = U @ D @ Vt
    scale = (S[:, 0] + S[:, 1] * sign) / var
    M = np.empty((n, 2, 3))
    M[:, :, :2] = R * scale[:, None, None]
    M[:, :, 2] = dst_mean - np.einsum("nij,nj->ni", M[:, :, :2], src_mean)
    if not np.isfinite(M).all() or (scale <= 0).any():
        raise ValueError("degenerate landmarks: no similarity transform fits them")
    return M


def invert_affine(M):
    """(…, 2, 3) -> (…, 2, 3), the inverse map by the adjugate formula, in float64 — the arithmetic of cv2.warpAffine without
    WARP_INVERSE_MAP: D = m00 m11 - m01 m10, D = 1 / D (0 when D is 0), A = [[m11 D, -m01 D], [-m10 D, m00 D]], b = -A t."""
    M = np.asarray(M, dtype=np.float64)
    if M.shape[-2:] != (2, 3):
        raise ValueError("expected (..., 2, 3) matrices, got %s" % (M.shape,))
    D = M[..., 0, 0] * M[..., 1, 1] - M[..., 0, 1] * M[..., 1, 0]
    with np.errstate(divide="ignore"):
        D = np.where(D != 0, 1.0 / np.where(D != 0, D, 1.0), 0.0)
    out = np.empty(M.shape)
    a00, a01 = M[..., 1, 1] * D, -M[..., 0, 1] * D
    a10, a11 = -M[..., 1, 0] * D, M[..., 0, 0] * D
    out[..., 0, 0], out[..., 0, 1], out[..., 1, 0], out[..., 1, 1] = a00, a01, a10, a11
    out[..., 0, 2] = -(a00 * M[..., 0, 2] + a01 * M[..., 1, 2])
    out[..., 1, 2] = -(a10 * M[..., 0, 2] + a11 * M[..., 1, 2])
    return out


def crop_box(shape, bbox=None, margin=44):
    """The box the reference crops before it resizes (code/face_preprocess.py:76-91): (x0, y0, x1, y1), half-open.
    shape = (H, W, ...) of the photo; bbox = (x0, y0, x1, y1) of the face, or None for the centre crop that leaves
    int(6.25 %) of each side out; either is widened by margin // 2 on every side and clipped to the photo; fractions are
    truncated as the reference's int32 assignment truncates them.  ValueError when nothing is left."""
    H, W = int(shape[0]), int(shape[1])
    if bbox is None:
        dx, dy = int(W * 0.0625), int(H * 0.0625)
        det = (dx, dy, W - dx, H - dy)
    else:
        det = np.asarray(bbox, dtype=np.float64).reshape(-1)
        if det.shape != (4,) or not np.isfinite(det).all():
            raise ValueError("a face box is four finite numbers (x0, y0, x1, y1), got %r" % (bbox,))
    half = int(margin) // 2
    bb = (int(max(det[0] - half, 0)), int(max(det[1] - half, 0)), int(min(det[2] + half, W)), int(min(det[3] + half, H)))
    if H < 1 or W < 1 or bb[0] >= bb[2] or bb[1] >= bb[3]:
        raise ValueError("face box %r leaves nothing of a %d x %d photo" % (bbox, W, H))
    return bb


def _per_image(arg, n, what):
    if arg is None:
        return [None] * n
    if len(arg) != n:
        raise ValueError("%d %s for %d images" % (len(arg), what, n))
    return list(arg)


def preprocess_batch_device(images, bboxes=None, landmarks=None, image_size=(112, 112), margin=44, layout="NHWC", device=None):
    """preprocess_batch, the faces left on the GPU: a CUDA float32 tensor (n, Ho, Wo, C) — (n, C, Ho, Wo) for layout="NCHW"."""
    import torch
    Ho, Wo = _size(image_size)
    if layout not in ("NHWC", "NCHW"):
        raise ValueError("layout must be NHWC or NCHW, got %r" % (layout,))
    n = len(images)
    boxes, marks = _per_image(bboxes, n, "boxes"), _per_image(landmarks, n, "landmark sets")
    imgs = []
    for i, im in enumerate(images):
        a = np.asarray(im.detach().cpu() if hasattr(im, "detach") else im)
        if a.ndim != 3 or min(a.shape) < 1:
            raise ValueError("image %d: expected a non-empty (H, W, C) array, got shape %s" % (i, a.shape))
        if imgs and a.shape[2] != imgs[0].shape[2]:
            raise ValueError("image %d has %d channels, image 0 has %d" % (i, a.shape[2], imgs[0].shape[2]))
        imgs.append(a if a.dtype == np.uint8 else a.astype(np.float32, copy=False))
    device = _abi.resolve_device(device)
    dev = torch.device("cuda", device)
    Cc = imgs[0].shape[2] if imgs else 3
    shape = (n, Ho, Wo, Cc) if layout == "NHWC" else (n, Cc, Ho, Wo)
    if n == 0:
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    as_u8 = all(a.dtype == np.uint8 for a in imgs)
    elem = 1 if as_u8 else 4
    # every descriptor is decided, and every box and matrix checked, before anything is uploaded or launched
    desc = np.zeros(n, _DESC)
    with_marks = [i for i in range(n) if marks[i] is not None]
    if with_marks:
        try:
            fwd = estimate_similarity(np.stack([np.asarray(marks[i], dtype=np.float64) for i in with_marks]), (Ho, Wo))
        except ValueError as ex:
            raise ValueError("landmarks: %s" % ex)
        inv = invert_affine(fwd)
        if not np.isfinite(inv).all():
            raise ValueError("landmarks give a transform that cannot be inverted")
        desc["mode"][with_marks] = 1
        desc["m"][with_marks] = inv.reshape(-1, 6)
    for i, a in enumerate(imgs):
        desc["H"][i], desc["W"][i] = a.shape[0], a.shape[1]
        if marks[i] is None:
            desc["box"][i] = crop_box(a.shape, boxes[i], margin)
    lib = _abi.init(device)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    stream = _abi.current_stream(device)
    lo = 0
    while lo < n:
        hi, total = lo, 0
        while hi < n and (hi == lo or (total + imgs[hi].size) * elem <= TABLE_BYTES):
            desc["offset"][hi] = total
            total += imgs[hi].size
            hi += 1
        host = torch.empty(total, dtype=torch.uint8 if as_u8 else torch.float32, pin_memory=True)
        table = host.numpy()
        for i in range(lo, hi):
            o = int(desc["offset"][i])
            table[o:o + imgs[i].size] = imgs[i].reshape(-1)
        d_table = host.to(dev, non_blocking=True)
        d_desc = torch.from_numpy(desc[lo:hi].view(np.uint8).reshape(-1)).to(dev)
        _abi.check(lib.alink_ingest_faces(_abi.ptr(d_table), 0 if as_u8 else 1, total, _abi.ptr(d_desc), hi - lo, Cc, Ho, Wo,
                                          0 if layout == "NHWC" else 1, _abi.ptr(out[lo:hi]), stream), "alink_ingest_faces")
        lo = hi
    return out


def preprocess_batch(images, bboxes=None, landmarks=None, image_size=(112, 112), margin=44, layout="NHWC", device=None):
    """Faces for a list of photos, each an (H, W, C) array of its own size, uint8 or float (RGB 0..255).
    bboxes / landmarks: None, or one entry per photo — a box (x0, y0, x1, y1) / five (x, y) points, or None.  A photo with
    landmarks is warped onto the template; else one with a box is cropped by crop_box(shape, box, margin) and resized; else
    crop_box's centre crop is.  image_size = (height, width) of the faces.
    Returns (n, Ho, Wo, C) float32 — (n, C, Ho, Wo) for layout="NCHW" — as a NumPy array, or as a CUDA tensor if any photo
    came as a torch tensor (noise.py's convention).  One upload and one launch per TABLE_BYTES of photos.  Raises ValueError,
    before anything is launched, for a box that leaves nothing of its photo or landmarks no similarity fits."""
    as_torch = any(hasattr(im, "detach") for im in images)
    out = preprocess_batch_device(images, bboxes, landmarks, image_size, margin, layout, device)
    return out if as_torch else out.cpu().numpy()


def preprocess(img, bbox=None, landmark=None, **kwargs):
    """The reference's call (code/face_preprocess.py:46): one (H, W, C) image -> the (Ho, Wo, C) float32 face.  kwargs:
    image_size ('112,112', the default here; the reference's '' — crop without a resize — is not offered), margin (44)."""
    if isinstance(img, str):
        raise TypeError("preprocess takes pixels; read the file first (PIL: np.asarray(Image.open(path).convert('RGB')))")
    image_size = kwargs.get('image_size', '112,112') or '112,112'
    return preprocess_batch([img], None if bbox is None else [bbox], None if landmark is None else [landmark],
                            image_size=image_size, margin=kwargs.get('margin', 44), device=kwargs.get('device'))[0]
