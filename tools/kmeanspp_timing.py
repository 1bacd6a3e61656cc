"""Time k-means++ seeding on the device (alink_kmeanspp, kmeanspp.hip) beside the ranked batch (alink_ranked_batch, batch.hip),
whose streaming pass moves the same bytes per pick, in the same process on the same rows.

    python tools/kmeanspp_timing.py [--rows 200000] [--emb 128] [--pool 12500] [--gallery 16] [--features 512] [--k 1024]
                                    [--repeats 9] [--host-rows 8192] [--host-picks 32] [--out profiles/r18a_kmeanspp_timing.json]

Two pools: `embedding_rows`, a (--rows, --emb) row table (the shape of the gradient embeddings of 200,000 pairs), and `pair_form`,
--pool x --gallery pairs of --features features formed on the fly from the two feature tables.  Every shape is warmed up
first; HIP events on the stream around whole calls; the two kernels alternate inside one loop; medians over --repeats, with
the minimum and maximum beside them.  Per pool and kernel: milliseconds per call at k and at k = 1, so microseconds per pick =
the difference over k - 1; the bytes a pick's lanes load (the rows, or both tables' rows per pair and the two index vectors;
the distances read and written; the ranked batch's utilities) and TB/s of them over the pick time.  `ratio_per_pick` is
k-means++ over ranked batch; `ranked_batch_spread` is max / min of the ranked batch's own repeats, the yardstick for whether
the ratio says anything.
  host   badge.kmeans_pp (float64 NumPy, one N x D distance pass per pick) on the first --host-rows embedding rows for
         --host-picks picks, host clock; a whole call at --rows and k is EXTRAPOLATED from it (time per pick scales with the
         rows) and named so.
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
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--emb", type=int, default=128)
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-rows", type=int, default=8192)
    ap.add_argument("--host-picks", type=int, default=32, help="picks of the host form to time (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18a_kmeanspp_timing.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "kmeanspp_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import badge, batch as B

    k = a.k
    gen = torch.Generator(device="cuda")
    gen.manual_seed(18)
    emb = torch.randn((a.rows, a.emb), generator=gen, device="cuda")
    n, g, D = a.pool, a.gallery, a.features
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    uniforms = np.random.RandomState(18).random_sample(k)
    pools = {"embedding_rows": (emb, a.rows, a.emb, 4 * a.rows * a.emb),
             "pair_form": ((left, right, li, ri), n * g, D, 2 * 4 * n * g * D + 2 * 4 * n * g)}
    res = {"k": k, "repeats": a.repeats}
    for name, (rows, N, Dn, row_bytes) in pools.items():
        utility = torch.rand(N, generator=gen, device="cuda")
        labeled = (emb[:1] if name == "embedding_rows" else (left[:1] - right[:1]).abs()).contiguous()
        runs = {"kmeanspp": lambda kk: badge.kmeans_pp_device(rows, kk, uniforms=uniforms[:kk]),
                "ranked_batch": lambda kk: B.ranked_batch_device(rows, utility, labeled, kk)}
        times = {kind: {"k": [], "k1": []} for kind in runs}
        for it in range(1 + a.repeats):                    # the first walk warms every kernel up
            for kind, fn in runs.items():
                ms1, _ = _call_ms(lambda: fn(1))
                ms, out = _call_ms(lambda: fn(k))
                if it:
                    times[kind]["k"].append(ms)
                    times[kind]["k1"].append(ms1)
                elif kind == "kmeanspp":
                    picks = out[0].cpu().numpy()
        per = {"kmeanspp": row_bytes + 2 * 4 * N, "ranked_batch": row_bytes + 3 * 4 * N}   # d2 read and written; the utilities
        entry = {"N": N, "D": Dn, "distinct_picks": int(len(set(picks.tolist()))), "picks_left_out": int((picks < 0).sum())}
        for kind in runs:
            call, call1 = float(np.median(times[kind]["k"])), float(np.median(times[kind]["k1"]))
            pick_us = 1e3 * (call - call1) / max(k - 1, 1)
            entry[kind] = {"ms_per_call": round(call, 3), "ms_per_call_min": round(float(np.min(times[kind]["k"])), 3),
                           "ms_per_call_max": round(float(np.max(times[kind]["k"])), 3), "ms_at_k1": round(call1, 3),
                           "us_per_pick": round(pick_us, 2), "bytes_per_pick_loaded": per[kind],
                           "TBps_loaded": round(per[kind] / (pick_us * 1e-6) / 1e12, 3)}
        entry["ratio_per_pick"] = round(entry["kmeanspp"]["us_per_pick"] / entry["ranked_batch"]["us_per_pick"], 3)
        entry["ranked_batch_spread"] = round(entry["ranked_batch"]["ms_per_call_max"] / entry["ranked_batch"]["ms_per_call_min"], 3)
        res[name] = entry
    if a.host_picks > 0:
        hr = min(a.host_rows, a.rows)
        Xh = emb[:hr].cpu().numpy()
        t0 = time.perf_counter()
        got, _ = badge.kmeans_pp(Xh, a.host_picks, uniforms[:a.host_picks])
        per_pick = (time.perf_counter() - t0) / a.host_picks
        dev_idx, _ = badge.kmeans_pp_device(emb[:hr].contiguous(), a.host_picks, uniforms=uniforms[:a.host_picks])
        res["host"] = {"rows": hr, "D": a.emb, "picks_timed": a.host_picks, "ms_per_pick": round(1e3 * per_pick, 3),
                       "s_per_call_extrapolated": round(per_pick * (a.rows / float(hr)) * k, 1),
                       "extrapolated_to": {"N": a.rows, "k": k},
                       "picks_shared_with_device": int((got == dev_idx.cpu().numpy()).sum())}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
