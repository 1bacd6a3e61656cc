"""CPU references for the raw-photo front end (a-link_amd/face_preprocess.py, csrc/ingest.hip), shared by
tests/test_face_preprocess_host.py and tests/test_gpu_ingest.py.  NumPy only; nothing here imports the package."""
import numpy as np


def warp_restatement(img, m, Ho, Wo):
    """Mode 1 of alink_ingest_faces as include/alink_hip.h states it, in NumPy float64: img (H, W, C) of any real dtype,
    m the six numbers that map an OUTPUT pixel to source coordinates -> (Ho, Wo, C) float32."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    m = [np.float64(v) for v in m]
    oy, ox = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    sx = (ox * m[0] + oy * m[1]) + m[2]
    sy = (ox * m[3] + oy * m[4]) + m[5]
    inside = (sx > -1.0) & (sx < W) & (sy > -1.0) & (sy < H)
    sx, sy = np.where(inside, sx, 0.0), np.where(inside, sy, 0.0)
    xf, yf = np.floor(sx), np.floor(sy)
    wx0, wy0 = 1.0 - (sx - xf), 1.0 - (sy - yf)
    wx1, wy1 = 1.0 - wx0, 1.0 - wy0
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)

    def tap(y, x):
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        v = img[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.float64)
        return np.where(ok[..., None], v, 0.0)

    t = np.zeros((Ho, Wo, img.shape[2]), np.float64)
    t = t + (tap(yi, xi) * wy0[..., None]) * wx0[..., None]
    t = t + (tap(yi, xi + 1) * wy0[..., None]) * wx1[..., None]
    t = t + (tap(yi + 1, xi) * wy1[..., None]) * wx0[..., None]
    t = t + (tap(yi + 1, xi + 1) * wy1[..., None]) * wx1[..., None]
    return np.where(inside[..., None], t, 0.0).astype(np.float32)


def warp_scipy(img, m, Ho, Wo):
    """the same through scipy.ndimage.affine_transform, channel by channel (rows are scipy's first axis)"""
    from scipy import ndimage
    img = np.asarray(img)
    return np.stack([ndimage.affine_transform(img[..., ch].astype(np.float64), [[m[4], m[3]], [m[1], m[0]]], offset=[m[5], m[2]],
                                              output_shape=(Ho, Wo), order=1, mode="grid-constant", cval=0, output=np.float32)
                     for ch in range(img.shape[2])], axis=-1)


def random_similarity(rng, H, W, Ho, Wo):
    """an output -> source similarity whose source footprint lies around the image, partly outside it"""
    th = rng.uniform(-np.pi, np.pi)
    s = rng.uniform(0.3, 1.5) * max(H, W) / float(max(Ho, Wo))
    a, b = s * np.cos(th), s * np.sin(th)
    cx, cy = rng.uniform(-0.2, 1.2) * W, rng.uniform(-0.2, 1.2) * H          # where the output's centre lands
    ox, oy = (Wo - 1) / 2.0, (Ho - 1) / 2.0
    return [a, -b, cx - (a * ox - b * oy), b, a, cy - (b * ox + a * oy)]


def closed_form_similarity(src, dst):
    """Least-squares 2-D similarity src -> dst without an SVD: on demeaned points a = sum(s . d) / sum |s|^2,
    b = sum(s x d) / sum |s|^2, M = [[a, -b], [b, a]], t = mean(d) - M mean(s).  -> (2, 3) float64"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    sm, dm = src.mean(axis=0), dst.mean(axis=0)
    s, d = src - sm, dst - dm
    den = (s ** 2).sum()
    a = (s * d).sum() / den
    b = (s[:, 0] * d[:, 1] - s[:, 1] * d[:, 0]).sum() / den
    A = np.array([[a, -b], [b, a]])
    return np.concatenate([A, (dm - A @ sm)[:, None]], axis=1)
