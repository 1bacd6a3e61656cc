"""Decoded photos -> network-sized faces: the ragged launch against one resize call per file, printed as one JSON line.

1,000 synthetic uint8 photos of 200 to 400 pixels a side (what a decoded DFW file is) become 112 x 112 float32 faces in host
memory, as the loaders need them, by
  * per_file:  noise.resize_images(photo.astype(float32)[None], (112, 112)) once per photo — the loaders' form before
               face_preprocess existed: a float32 upload, a launch, a download and a synchronisation per file;
  * ragged:    ONE face_preprocess.preprocess_batch over all of them (whole-photo boxes, margin 0): one pinned uint8 table,
               one upload, one launch of alink_ingest_faces, one download.
The two give the same bytes (checked here before anything is timed).  Host clock around calls that end in the download,
after one full untimed pass of each; `--reps` timed passes of each, ALTERNATING, so that whatever else the host is doing
falls on both; median, fastest and slowest are reported in files per second.  Also: the same call with five landmarks per
photo (the alignment warp), and the two kernels alone under HIP events with their table already on the device.

    python tools/ingest_time.py [--files 1000] [--reps 7] > profiles/<name>.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "a timing needs the GPU"
    import a_link_amd  # noqa: F401
    from a_link_amd import _abi, face_preprocess as FP, noise
    rng = np.random.RandomState(0)
    n = args.files
    photos = [rng.randint(0, 256, (rng.randint(200, 401), rng.randint(200, 401), 3)).astype(np.uint8) for _ in range(n)]
    full = [(0, 0, p.shape[1], p.shape[0]) for p in photos]
    marks = [FP.template() * rng.uniform(0.8, 2.0) + [rng.uniform(0, 0.3) * p.shape[1], rng.uniform(0, 0.3) * p.shape[0]]
             for p in photos]

    def per_file():
        return np.stack([np.asarray(noise.resize_images(p.astype(np.float32)[None], (112, 112)))[0] for p in photos])

    def ragged():
        return FP.preprocess_batch(photos, bboxes=full, margin=0)

    def ragged_warp():
        return FP.preprocess_batch(photos, landmarks=marks)

    forms = (("per_file", per_file), ("ragged", ragged), ("ragged_warp", ragged_warp))
    first = {name: fn() for name, fn in forms}                       # the untimed pass: code objects, allocator, pinned pool
    assert first["per_file"].tobytes() == first["ragged"].tobytes(), "the two forms must give the same faces"
    secs = {name: [] for name, _ in forms}
    for _ in range(args.reps):
        for name, fn in forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            secs[name].append(time.perf_counter() - t0)
    out = {"files": n, "photo_sides": [200, 400], "photo_megabytes_uint8": round(sum(p.size for p in photos) / 1e6, 1),
           "face": [112, 112, 3], "reps": args.reps, "timer": "host clock around calls that end in the download; HIP events for the kernels",
           "device": torch.cuda.get_device_name(0), "identical_faces": True}
    for name, _ in forms:
        s = sorted(secs[name])
        out[name] = {"files_per_s_median": round(n / s[len(s) // 2], 1), "files_per_s_fastest": round(n / s[0], 1),
                     "files_per_s_slowest": round(n / s[-1], 1), "ms_median": round(1e3 * s[len(s) // 2], 2)}
    out["ragged_over_per_file"] = round(out["ragged"]["files_per_s_median"] / out["per_file"]["files_per_s_median"], 2)

    # the kernels alone: table and descriptors already on the device
    lib = _abi.init(0)
    table = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).cuda()
    faces = torch.empty((n, 112, 112, 3), dtype=torch.float32, device="cuda")
    inv = FP.invert_affine(FP.estimate_similarity(np.stack(marks)))
    for name, mode in (("crop_resize", 0), ("warp", 1)):
        d = np.zeros(n, FP._DESC)
        d["offset"] = np.concatenate([[0], np.cumsum([p.size for p in photos])[:-1]])
        d["H"], d["W"] = [p.shape[0] for p in photos], [p.shape[1] for p in photos]
        d["mode"], d["box"], d["m"] = mode, full, inv.reshape(n, 6)
        d_desc = torch.from_numpy(d.view(np.uint8).reshape(-1)).cuda()

        def launch():
            _abi.check(lib.alink_ingest_faces(_abi.ptr(table), 0, table.numel(), _abi.ptr(d_desc), n, 3, 112, 112, 0, _abi.ptr(faces),
                                              _abi.current_stream(0)), "alink_ingest_faces")
        for _ in range(3):
            launch()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(50):
            launch()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 50
        out["kernel_" + name] = {"ms": round(ms, 4), "faces_per_s": round(n / ms * 1e3), "GBps_faces_written": round(faces.numel() * 4 / ms / 1e6, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
