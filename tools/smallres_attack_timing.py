"""Time the few-pixel attack on the SmallRes student (PixelAttacker.attack_all over noise.PredictionWrappedModel(SmallRes, None)).

    python tools/smallres_attack_timing.py --source 48 --route pixel --lockstep 32
    python tools/smallres_attack_timing.py --source 48 --route generic            # the route before the pixel scorer existed
    python tools/smallres_attack_timing.py --source 224 --route pixel --lockstep 32

8 pairs, the reference's search settings (40 pixels, 50 generations, popsize 250: code/attack.py:91), early_stop=False, a 48 x 48
student with 2048 features.  --route generic hides the student behind an object that offers `predict` only, which is what sends
attack_all down the reference-shaped route (perturb on the device, candidates to the host, SmallRes.predict); that route is only
right when the source is the student's size.  Prints one JSON line: seconds per pair, pair-forwards per second (nfev / time),
the peak device memory of the timed call.  For the device-time split run it once under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class PredictOnly(object):
    """the student as a duck-typed model: nothing but predict (the generic route's whole contract)"""

    def __init__(self, model):
        self._m = model

    def predict(self, X):
        return self._m.predict(X)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--source", type=int, default=48, help="side of the source images (the stacked pair is 2s x s)")
    ap.add_argument("--student", type=int, default=48)
    ap.add_argument("--route", choices=("pixel", "generic"), default="pixel")
    ap.add_argument("--lockstep", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--pixels", type=int, default=40)
    ap.add_argument("--maxiter", type=int, default=50)
    ap.add_argument("--popsize", type=int, default=250)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--early_stop", action="store_true", help="keep the success test (the generic route then runs its second forward "
                    "per generation, as it always did before attack_all's early_stop reached it)")
    a = ap.parse_args(argv)
    import torch
    import a_link_amd  # noqa: F401
    from a_link_amd import attack as A, noise as N, siamese
    student = siamese.SmallRes((a.student, a.student, 3), (2048,), "timing", 0.1, seed=1)
    wrapped = N.PredictionWrappedModel(student if a.route == "pixel" else PredictOnly(student), None)
    if a.route == "generic" and a.source != a.student:
        raise SystemExit("the generic route reads the student's size only")
    rng = np.random.RandomState(0)
    s = a.source
    imgs = [rng.randint(0, 256, (2 * s, s, 3)).astype(np.float32) for _ in range(a.pairs)]
    targets = [[0, 1] if i % 2 else [1, 0] for i in range(a.pairs)]
    kw = dict(dimensions=(2 * s, s), pixel_count=a.pixels, popsize=a.popsize, seeds=list(range(50, 50 + a.pairs)), early_stop=a.early_stop)
    att = A.PixelAttacker(wrapped, lockstep=a.lockstep if a.route == "pixel" else 0)
    att.attack_all(imgs[:2], targets[:2], maxiter=2, **kw)                    # warm-up: allocations, first launches
    torch.cuda.synchronize()
    times, mem = [], 0
    for _ in range(a.repeats):
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        att.attack_all(imgs, targets, maxiter=a.maxiter, **kw)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        mem = max(mem, torch.cuda.max_memory_allocated())
    nfev = int(sum(r.nfev for r in att.last_results))
    t = float(np.median(times))
    print(json.dumps({"route": a.route, "lockstep": a.lockstep if a.route == "pixel" else 0, "source": s, "student": a.student,
                      "pairs": a.pairs, "pixels": a.pixels, "early_stop": a.early_stop, "maxiter": a.maxiter, "popsize": a.popsize,
                      "generations": [int(r.nit) for r in att.last_results], "pair_forwards": nfev,
                      "seconds": [round(x, 4) for x in times], "seconds_per_pair": round(t / a.pairs, 4),
                      "pair_forwards_per_second": round(nfev / t, 1), "peak_device_MB": round(mem / 2 ** 20, 1)}))


if __name__ == "__main__":
    main()
