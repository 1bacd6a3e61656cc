"""Time of SmallRes' input-gradient pass next to predict and train_on_batch, printed as one JSON line.

Per size — 16 and 256 pairs at 32 x 32 / 2048 and at 48 x 48 / 2048, device operands — in ONE process: input_gradients, predict
and train_on_batch, each as the median of --rounds windows of --reps calls after warm-up (wall clock around a window that ends
with a device synchronisation; the three interleaved so that drift hits them alike), with the windows' spread.  Then ONE
`rocprofv3 --kernel-trace --stats` run of a fresh child process (this file with --child) gives the device time of the two new
kernels — conv1_dgrad_kernel per size, resize_grad_kernel at 64 x 64 -> 32 x 32 for 16 and 256 images — and conv1_dgrad_kernel's
achieved fraction of its traffic floor: 128 B read + 12 B written per pixel against --hbm_tbs (6.3 TB/s achievable on MI355X).

    python tools/smallres_grad_timing.py [--reps 10] [--rounds 7] [--no_profile] > profiles/<name>.json
"""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(32, 2048, 16), (32, 2048, 256), (48, 2048, 16), (48, 2048, 256)]          # (image side, features, pairs)
RESIZE_IMAGES = [16, 256]
CHILD_WARM, CHILD_CALLS = 3, 20


def _operands(size, n, seed=0):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    L = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3)).astype(np.float32)).cuda()
    R = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3)).astype(np.float32)).cuda()
    y = torch.from_numpy(np.eye(2, dtype=np.float32)[rng.integers(0, 2, n)]).cuda()
    return L, R, y


def _model(size, feat):
    from a_link_amd.smallres import SmallResNet
    return SmallResNet((size, size, 3), feat, lr=0.1, seed=3, prescale=True)


def child():
    """what the profiler sees: per size CHILD_WARM + CHILD_CALLS gradient passes, then as many resize adjoints per image count —
    in this order, so that the trace's launches of a kernel, sorted by start, fall into blocks of one configuration each"""
    import torch
    from a_link_amd import noise
    for size, feat, n in SIZES:
        net = _model(size, feat)
        L, R, y = _operands(size, n)
        for _ in range(CHILD_WARM + CHILD_CALLS):
            net.input_gradients([L, R], y, reduction="sum")
        torch.cuda.synchronize()
        del net
    for n in RESIZE_IMAGES:
        g = torch.randn((n, 32, 32, 3), device="cuda")
        for _ in range(CHILD_WARM + CHILD_CALLS):
            noise.resize_images_grad(g, (64, 64))
        torch.cuda.synchronize()


def _window_us(fn, reps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def _profile(timeout):
    """median device microseconds per configuration of the two new kernels, from one kernel trace of a child process"""
    out = tempfile.mkdtemp(prefix="smallres_grad_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--child"]
        subprocess.run(cmd, check=True, timeout=timeout, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=out)
        dbs = glob.glob(os.path.join(out, "**", "*.db"), recursive=True)
        assert dbs, "the profiler wrote no database under %s" % out
        c = sqlite3.connect(dbs[0])
        res = {}
        for key, configs in (("conv1_dgrad_kernel", SIZES), ("resize_grad_kernel", RESIZE_IMAGES)):
            d = [r[0] / 1e3 for r in c.execute("select duration from kernels where name like ? order by start", ("%" + key + "%",))]
            per = CHILD_WARM + CHILD_CALLS
            assert len(d) == per * len(configs), "%s: %d launches in the trace, expected %d" % (key, len(d), per * len(configs))
            res[key] = [statistics.median(d[i * per + CHILD_WARM:(i + 1) * per]) for i in range(len(configs))]
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--hbm_tbs", type=float, default=6.3)
    ap.add_argument("--no_profile", action="store_true")
    ap.add_argument("--profile_timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    import a_link_amd  # noqa: F401
    if args.child:
        return child()
    assert args.rounds >= 5
    sizes = []
    for size, feat, n in SIZES:
        net = _model(size, feat)
        L, R, y = _operands(size, n)
        fns = {"input_gradients": lambda: net.input_gradients([L, R], y, reduction="sum"),
               "predict": lambda: net.predict([L, R]),
               "train_on_batch": lambda: net.train_on_batch([L, R], y)}
        for f in fns.values():
            for _ in range(3):
                f()
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, f in fns.items():
                t[k].append(_window_us(f, args.reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = max(max(v) - min(v) for v in (t["input_gradients"], t["train_on_batch"]))
        sizes.append({"image": size, "feat": feat, "pairs": n,
                      "us": {k: round(v, 1) for k, v in med.items()},
                      "spread_us": {k: [round(min(v), 1), round(max(v), 1)] for k, v in t.items()},
                      "gradient_over_train_step": round(med["input_gradients"] / med["train_on_batch"], 3),
                      "gradient_no_slower_than_train_step": bool(med["input_gradients"] <= med["train_on_batch"] + spread)})
        del net
    res = {"tool": "smallres_grad_timing", "device": torch.cuda.get_device_name(0), "measured": True,
           "timer": "wall clock around windows ending in a device synchronisation", "reps": args.reps, "rounds": args.rounds,
           "operands": "device", "sizes": sizes}
    if not args.no_profile:
        prof = _profile(args.profile_timeout)
        for s, us in zip(sizes, prof["conv1_dgrad_kernel"]):
            pixels = 2 * s["pairs"] * s["image"] * s["image"]
            floor_us = pixels * 140 / (args.hbm_tbs * 1e12) * 1e6
            s["conv1_dgrad_kernel_us"] = round(us, 2)
            s["conv1_dgrad_traffic_floor_us"] = round(floor_us, 2)
            s["conv1_dgrad_fraction_of_floor"] = round(floor_us / us, 3)
        res["resize_grad_kernel_us"] = {"64x64->32x32, %d images" % n: round(us, 2) for n, us in zip(RESIZE_IMAGES, prof["resize_grad_kernel"])}
        res["kernel_timer"] = "rocprofv3 --kernel-trace --stats, one child process, median of %d launches per configuration" % CHILD_CALLS
    print(json.dumps(res))


if __name__ == "__main__":
    main()
