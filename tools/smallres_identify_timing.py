"""Time top-1 identification on the SmallRes student: the pair route (alink_loop.top1_identification: P x G pixel pairs built on the
host, the tower on every pair occurrence) against the gallery route (alink_loop.top1_identification_gallery: every face embedded
once, the pair head on the P x G feature pairs, each probe's argmax on the device), on the same synthetic split.

    python tools/smallres_identify_timing.py --people 64 --images 8 --size 48 --feat 2048

Each route runs in a process of its own under its own time limit (--timeout seconds), one after the other; the first one that
fails, faults or runs out of time ends the tool with its status and nothing further is started.  A route is warmed up once (every
shape it uses), then timed --repeats times with a host clock around the whole call (it ends in a device-to-host copy); the gallery
route also reports its split — tower (features of gallery and probes), head (score_matrix), reduce (identify_rows) — from device
events around one more walk.  Prints one JSON line: both routes' seconds, the pair count, the two accuracies.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _split(a):
    rng = np.random.RandomState(a.seed)
    return [rng.randint(0, 256, (a.images, a.size, a.size, 3)).astype(np.float32) for _ in range(a.people)]


def _student(a):
    from a_link_amd import siamese
    student = siamese.SmallRes((a.size, a.size, 3), (a.feat,), "timing", 0.1, seed=1)
    ws = student.siamese_net.get_weights()
    ws[14] = ws[14] * np.float32(8.0)                    # scores spread away from 0.5
    student.siamese_net.set_weights(ws)
    return student


def _timed(fn, repeats):
    import torch
    acc = fn()                                           # warm-up: allocations, first launches of every shape
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        acc = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return acc, times


def run_route(a):
    import torch
    import a_link_amd  # noqa: F401
    from a_link_amd import alink_loop, smallres
    student, people = _student(a), _split(a)
    res = {"route": a.route}
    if a.route == "pair":
        acc, times = _timed(lambda: alink_loop.top1_identification(student, people), a.repeats)
    else:
        acc, times = _timed(lambda: alink_loop.top1_identification_gallery(student, people), a.repeats)
        # the split, from device events around one direct walk (inputs already on the device: the kernels alone)
        net = student.siamese_net
        probes, ids, gallery = alink_loop._gallery_split(people)
        pd, gd = torch.from_numpy(probes).cuda(), torch.from_numpy(gallery).cuda()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for _ in range(2):                               # (the first walk warms these shapes up)
            ev[0].record()
            FG, FP = net.features(gd, prescale=True), net.features(pd, prescale=True)
            ev[1].record()
            sc = net.score_matrix(FP, FG)
            ev[2].record()
            smallres.identify_rows(sc, col=1, true_ids=ids)
            ev[3].record()
            torch.cuda.synchronize()
        res["device_ms"] = {k: round(ev[i].elapsed_time(ev[i + 1]), 4) for i, k in enumerate(("tower", "head", "reduce"))}
    res.update(accuracy=acc, seconds=[round(t, 5) for t in times], median_seconds=round(float(np.median(times)), 5))
    print(json.dumps(res))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--people", type=int, default=64)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=48)
    ap.add_argument("--feat", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--timeout", type=int, default=240, help="seconds each route's process may take")
    ap.add_argument("--route", choices=("pair", "gallery"), default=None, help="run this route alone, in this process")
    a = ap.parse_args(argv)
    if a.route:
        return run_route(a)
    out = {"people": a.people, "images": a.images, "size": a.size, "feat": a.feat, "probes": a.people * a.images, "gallery_faces": a.people,
           "pairs": a.people * a.images * a.people}
    for route in ("pair", "gallery"):
        cmd = [sys.executable, os.path.abspath(__file__), "--route", route] + [x for k in ("people", "images", "size", "feat", "repeats", "seed")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit("the %s route did not finish in %d s: stopping" % (route, a.timeout))
        if p.returncode != 0:
            raise SystemExit("the %s route ended with status %d: stopping" % (route, p.returncode))
        out[route] = json.loads(p.stdout.decode().strip().splitlines()[-1])
    out["pair_over_gallery"] = round(out["pair"]["median_seconds"] / out["gallery"]["median_seconds"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
