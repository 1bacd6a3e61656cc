"""readDFW — drop-in for the parts of reference code/readDFW.py the drivers call.

    lookupFile(fullPath)                                          code/readDFW.py:8-26
    constructIndexMap(filePath)                                   code/readDFW.py:47-53
    getAllTrainData(prefix, trainFolder, imageRes, model, ...)    code/readDFW.py:65-105
    getRawTrainData(prefix, trainFolder, imageRes)                code/readDFW.py:108-140
    getNormalGenerator / getImposterGenerator / getGenerator /
    splitDisguiseData / createMiniBatch                           code/readDFW.py:143-244   (pairs.py)

DFW layout: <prefix>/<trainFolder>/<person>/<files>; a file name containing `_h_` is a disguised face,
`_I_` an impersonator, anything else a plain face of that person.  Images are read with PIL as RGB
0..255 and resized to imageRes with the bilinear rule of cv2.resize on the device: every file has its
own size, and all of them go through one ragged launch (face_preprocess.preprocess_batch ->
alink_ingest_faces) per 1,024 files.  A person is kept only if it has all the kinds the reference asks
for; unreadable files are reported and skipped.
DFW is distributed as whole photos plus a face-coordinate file.  The reference crops by rewriting the
image files in place (cropImages / cropAllFolders, code/readDFW.py:28-62: PIL's Image.crop, then
save); here the files stay as distributed and the loaders take `faceBoxes=constructIndexMap(file)`:
the crop happens in the same launch as the resize.  Box coordinates are rounded as Image.crop rounds
them and CLIPPED to the photo, where PIL pads a box that sticks out of it with black; the reference
also re-encodes the crop in the photo's own (usually JPEG) format before it is read again, which this
does not reproduce.
"""
import os
import re

import numpy as np

from .pairs import (createMiniBatch, getGenerator, getImposterGenerator, getNormalGenerator,  # noqa: F401
                    splitDisguiseData)

_BOM = '\xef\xbb\xbf'          # DFW's file lists carry stray byte-order marks in directory / file names


def lookupFile(fullPath):
    """The path itself or one of the BOM / leading-blank variants DFW ships (None if none exists)."""
    directory, fileName = fullPath.rsplit('/', 1)
    stem, extension = fileName.rsplit('.', 1)
    candidates = [fullPath,
                  os.path.join(directory + _BOM, stem) + "." + extension,
                  os.path.join(directory + _BOM, stem + _BOM) + "." + extension,
                  os.path.join(directory, stem + _BOM) + "." + extension,
                  os.path.join(directory, " " + stem) + "." + extension]
    for c in candidates:
        if os.path.exists(c):
            return c
    print(fullPath)
    print(os.listdir(directory))
    return None


def constructIndexMap(filePath):
    """DFW's face-coordinate file (Training_data_face_coordinate.txt; code/readDFW.py:47-53) -> {relative file name:
    [left, upper, right, lower]}.  One photo per line, the name first — it may contain blanks — then four numbers."""
    mapping = {}
    with open(filePath, 'r') as f:
        for row in f:
            row = row.rstrip('\n').rstrip()
            if not row:
                continue
            name, left, upper, right, lower = row.rsplit(' ', 4)
            mapping[name] = [float(v) for v in (left, upper, right, lower)]
    return mapping


def _pil_box(box, H, W):
    """(left, upper, right, lower) -> (x0, y0, x1, y1) rounded as PIL's Image.crop rounds (int(round(v))) and clipped to the
    image; None when nothing is left.  PIL pads the part of a box that sticks out of the image with black; this clips."""
    x0, y0, x1, y1 = (int(round(v)) for v in box)
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


_FILES_PER_BATCH = 1024          # decoded photos held on the host at a time (DFW: ~300 KB each as uint8)


def load_resized(paths, imageRes, boxes=None):
    """cv2.resize(photo, imageRes) of every file in `paths` (imageRes = (width, height)) -> (list of float32 (H, W, 3) images,
    one per file that could be read, list of their positions in `paths`).  Two steps: the files are decoded with PIL (RGB,
    uint8), then every _FILES_PER_BATCH of them go through ONE face_preprocess.preprocess_batch — one upload and one launch
    whatever their sizes, where a per-file resize paid an upload, a launch, a download and a sync per file.  The pixels are
    those of noise.resize_images on each float32 photo, bit for bit.  boxes: None, or per file (left, upper, right, lower) —
    the photo is cropped to it (_pil_box) before the resize; a file whose box misses the photo is reported and skipped, as
    is an unreadable file."""
    from PIL import Image
    from . import face_preprocess
    images, kept = [], []
    for lo in range(0, len(paths), _FILES_PER_BATCH):
        photos, rects, idx = [], [], []
        for i in range(lo, min(len(paths), lo + _FILES_PER_BATCH)):
            try:
                img = np.asarray(Image.open(lookupFile(paths[i])).convert('RGB'))
                H, W = img.shape[:2]
                rect = (0, 0, W, H) if boxes is None else _pil_box(boxes[i], H, W)
                if rect is None:
                    raise ValueError("%s: face box %r lies outside the %d x %d photo" % (paths[i], boxes[i], W, H))
            except Exception as ex:
                print(ex)
                continue
            photos.append(img)
            rects.append(rect)
            idx.append(i)
        if photos:
            faces = face_preprocess.preprocess_batch(photos, bboxes=rects, image_size=(imageRes[1], imageRes[0]), margin=0)
            if faces.shape[1:] != (imageRes[1], imageRes[0], 3):
                raise SystemExit("Image re-shape error occured. Exiting!")
            images.extend(faces)
            kept.extend(idx)
    return images, kept


def _people(prefix, trainFolder, imageRes, faceBoxes=None):
    """Yields per person the three lists (plain, disguised, impersonator) of loaded images.  faceBoxes: {relative file name
    (trainFolder/person/file, the coordinate file's names) : (left, upper, right, lower)} — every photo is cropped to its
    box before the resize; a photo without an entry is reported and skipped (the reference's cropImages deletes such a
    file, code/readDFW.py:37-41)."""
    root = os.path.join(prefix, trainFolder)
    paths, boxes, owner = [], [], []
    persons = sorted(os.listdir(root))
    for p, person in enumerate(persons):
        dirPath = os.path.join(root, person)
        for impath in sorted(os.listdir(dirPath)):
            if faceBoxes is not None:
                key = os.path.join(trainFolder, person, impath)
                if key not in faceBoxes:
                    print("no face box for %s" % key)
                    continue
                boxes.append(faceBoxes[key])
            paths.append(re.sub(r"[/]\s", "/", os.path.join(dirPath, impath)))
            fileName = impath.rsplit('.', 1)[0]
            owner.append((p, "dig" if '_h_' in fileName else ("imp" if '_I_' in fileName else "plain")))
    images, kept = load_resized(paths, imageRes, boxes if faceBoxes is not None else None)
    people = [{"plain": [], "dig": [], "imp": []} for _ in persons]
    for img, i in zip(images, kept):
        people[owner[i][0]][owner[i][1]].append(img)
    for kinds in people:
        yield kinds


def getAllTrainData(prefix, trainFolder, imageRes, model, combine_normal_imp=False, faceBoxes=None):
    """-> (X_plain, X_dig, X_imp): per-person FEATURE arrays, model.process applied at load.  faceBoxes: see _people.
    combine_normal_imp files the disguised images under "plain" (code/readDFW.py:87-90); the keep-test
    that follows still asks for a non-empty disguised list (:97), so in that mode the reference — and
    this function — return no person at all (the baseline script that sets the flag, existing_al.py,
    cannot have worked on it).  Reproduced, not repaired."""
    # The reference embeds person by person (three model.process calls of one to three images each, code/readDFW.py:97-101: 1.5 ms of
    # launch latency per call here).  An embedding does not depend on the batch it is computed in (bit for bit: DESIGN.md §5), so the
    # kept persons' images are embedded in chunks of `chunk` and handed back per person — the same arrays, ~10x sooner at load.
    kept, chunk = [], 1024
    for k in _people(prefix, trainFolder, imageRes, faceBoxes):
        plain, dig = (k["plain"] + k["dig"], []) if combine_normal_imp else (k["plain"], k["dig"])
        if dig and k["imp"] and plain:
            kept.append(([] if combine_normal_imp else dig, k["imp"], plain))
    flat = [img for person in kept for part in person for img in part]
    feats = [model.process(np.stack(flat[s0:s0 + chunk])) for s0 in range(0, len(flat), chunk)]
    feats = np.concatenate([np.asarray(f) for f in feats]) if feats else None
    X_plain, X_dig, X_imp = [], [], []
    o = 0
    for dig, imp, plain in kept:
        if not combine_normal_imp:
            X_dig.append(feats[o:o + len(dig)].copy())
        o += len(dig)
        X_imp.append(feats[o:o + len(imp)].copy())
        o += len(imp)
        X_plain.append(feats[o:o + len(plain)].copy())
        o += len(plain)
    if not combine_normal_imp:
        assert len(X_plain) == len(X_dig) and len(X_dig) == len(X_imp)
    return (X_plain, X_dig, X_imp)


def getRawTrainData(prefix, trainFolder, imageRes, faceBoxes=None):
    """-> (X_plain, X_dig): per-person raw pixel arrays (k, H, W, 3).  A person needs disguised AND
    impersonator images (the reference's condition, code/readDFW.py:136, never looks at the plain list).
    faceBoxes: see _people."""
    X_plain, X_dig = [], []
    for k in _people(prefix, trainFolder, imageRes, faceBoxes):
        if k["dig"] and k["imp"]:
            X_dig.append(np.stack(k["dig"]))
            X_plain.append(np.stack(k["plain"]))
    assert len(X_plain) == len(X_dig)
    return (X_plain, X_dig)
