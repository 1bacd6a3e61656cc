"""Time ranked batch-mode selection on the device (alink_ranked_batch, batch.hip) at the per-GPU shape of BASELINE configs[2]:
12,500 pool x 16 gallery images = 200,000 pairs of 512 features, 4,096 labelled rows, a batch of 1,024.

    python tools/ranked_batch_timing.py [--pool 12500] [--gallery 16] [--features 512] [--labeled 4096] [--k 1024]
                                        [--repeats 5] [--host-picks 3] [--out profiles/r14a_ranked_batch_timing.json]

Both row forms on the same pool, alternating, every shape warmed up first, HIP events around whole calls (medians over --repeats):
  row form   batch.ranked_batch_device on the materialised (N, D) rows |left[li] - right[ri]|
  pair form  the same on (left, right, li, ri): rows formed on the fly from the two feature tables
Per form: milliseconds per call at k and at k = 1 (init + one pick), so microseconds per pick = the difference over k - 1; bytes
per pick from the shapes — `loaded`: what the lanes load (the rows, or both tables' rows per pair; the distances read and
written, the utilities), `unique`: each address once (the pair form's tables instead of its rows) — and TB/s of the loaded
bytes over the pick time.  The two forms' picks are compared (they must be the same) and counted against the plain top-k.
  host       batch.ranked_batch (float64 NumPy + sklearn, one pairwise_distances_argmin_min per pick) on the same input for
             --host-picks picks, host clock; a whole call is k such picks, so its time is EXTRAPOLATED from them and named so.
Writes one JSON (--out) and prints it.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _unit(t):
    return t / t.norm(dim=1, keepdim=True)


def _call_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--labeled", type=int, default=4096)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-picks", type=int, default=3, help="picks of the host form to time (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14a_ranked_batch_timing.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "ranked_batch_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import batch as B, uncertainty as U

    n, g, D, M, k = a.pool, a.gallery, a.features, a.labeled, a.k
    N = n * g
    gen = torch.Generator(device="cuda")
    gen.manual_seed(14)
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    rows = (left[li.long()] - right[ri.long()]).abs().contiguous()
    labeled = (_unit(torch.randn((M, D), generator=gen, device="cuda")) - _unit(torch.randn((M, D), generator=gen, device="cuda"))).abs()
    utility = torch.rand(N, generator=gen, device="cuda")

    forms = {"row_form": rows, "pair_form": (left, right, li, ri)}
    times = {name: {"k": [], "k1": []} for name in forms}
    picks = {}
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for name, r in forms.items():
            ms1, _ = _call_ms(lambda: B.ranked_batch_device(r, utility, labeled, 1))
            ms, out = _call_ms(lambda: B.ranked_batch_device(r, utility, labeled, k))
            picks[name] = out
            if it:
                times[name]["k"].append(ms)
                times[name]["k1"].append(ms1)
    same = bool(torch.equal(picks["row_form"][0], picks["pair_form"][0]) and torch.equal(picks["row_form"][1], picks["pair_form"][1]))
    top, _ = U.topk_device(utility, k)
    chosen = picks["row_form"][0].cpu().numpy()
    shared = 4 * N * 3                                     # distances read and written, utilities read
    nbytes = {"row_form": {"loaded": 4 * N * D + shared, "unique": 4 * N * D + shared},
              "pair_form": {"loaded": 2 * 4 * N * D + 2 * 4 * N + shared, "unique": 4 * (n + g) * D + 2 * 4 * N + shared}}
    res = {"shape": {"N": N, "D": D, "M": M, "k": k, "pool_images": n, "gallery_images": g}, "repeats": a.repeats,
           "forms_pick_the_same": same, "picks_outside_plain_topk": int(len(set(chosen.tolist()) - set(top.cpu().numpy().tolist())))}
    for name in forms:
        call, call1 = float(np.median(times[name]["k"])), float(np.median(times[name]["k1"]))
        pick_us = 1e3 * (call - call1) / max(k - 1, 1)
        res[name] = {"ms_per_call": round(call, 3), "ms_per_call_min": round(float(np.min(times[name]["k"])), 3),
                     "ms_init_and_one_pick": round(call1, 3), "us_per_pick": round(pick_us, 2),
                     "bytes_per_pick_loaded": nbytes[name]["loaded"], "bytes_per_pick_unique": nbytes[name]["unique"],
                     "TBps_loaded": round(nbytes[name]["loaded"] / (pick_us * 1e-6) / 1e12, 3)}
    if a.host_picks > 0:
        class _Labelled:
            X_training = labeled.cpu().numpy().astype(np.float64)
        Xh, uh = rows.cpu().numpy().astype(np.float64), utility.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        got = B.ranked_batch(_Labelled(), Xh, uh, a.host_picks, "euclidean", None)
        per_pick = (time.perf_counter() - t0) / a.host_picks
        res["host"] = {"picks_timed": a.host_picks, "s_per_pick": round(per_pick, 3), "s_per_call_extrapolated": round(per_pick * k, 1),
                       "same_first_picks_as_device": bool(np.array_equal(got, chosen[:a.host_picks]))}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
