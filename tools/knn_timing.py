"""Time the k-nearest-neighbour search on the device (alink_knn, knn.hip) beside what the library's user could do without it:
torch.matmul of a chunk of rows with the whole pool, the scores formed in place, torch.topk over each chunk — in the same process
on the same rows — and one end-to-end TypiClust call.

    python tools/knn_timing.py [--rows 200000] [--emb 128] [--pool 12500] [--gallery 16] [--features 512] [--k 20]
                               [--clusters 1024] [--repeats 5] [--yard-repeats 2] [--chunk 2048] [--instances 1024]
                               [--step-timeout 240] [--out profiles/r20a_knn_timing.json]

Without --step the tool touches no GPU itself: it runs each step — `embedding_rows`, `pair_form`, `typiclust` — as a fresh child
process under its own time limit (--step-timeout seconds), one after the other, stops at the first that fails or runs out of
time, and merges their JSON.  With --step NAME it runs that step in this process and prints its JSON.

Two pools: `embedding_rows`, a (--rows, --emb) row table, and `pair_form`, --pool x --gallery pairs of --features features formed
on the fly from the two feature tables.  Every shape is warmed up first; HIP events on the stream around whole calls; the two
forms of the fused call alternate inside one loop; medians over --repeats, with the minimum and maximum beside them.
  knn            alink_knn with every output (idx, d2, found, typicality), K = --k, no groups: the norms, the fused product + lists,
                 the distance pass.  TFLOP/s = 2 N^2 D over that whole time, against the 157.3 TFLOP/s f32 matrix peak — a
                 whole-call rate, not a kernel's: kmeans.hip's assignment, the same walk with a running minimum in place of the
                 lists, reaches 52 % of that peak, and the distance to it is the cost of the lists.
  knn_grouped    the same with groups = the assignment of cluster.kmeans_device into --clusters clusters (3 iterations): the same
                 walk (no tile is skipped), fewer insertions.
  matmul_topk    the yardstick: per chunk of --chunk rows torch.matmul(chunk, pool^T) into a (chunk, N) buffer, scores = |x_j|^2 -
                 2 P in place, the diagonal set to +inf, torch.topk(K, largest=False, sorted=True).  Indices only — no d2, no
                 typicality, no groups — so the fused call is compared with LESS work than it does.  The pair form has no row
                 table: it is materialised first (|left[li] - right[ri]| by torch), inside the timed region.
  `fused_over_yardstick` is knn over matmul_topk; `neighbour_sets_equal` the share of rows whose K indices, as sets, are the same
  in both (the yardstick's float32 GEMM sums in another order: near-ties may differ).
  typiclust      one typiclust.typiclust_device call on the embedding rows, n_instances = --instances, nothing labelled, host clock
                 around the call (it reads its picks back, which synchronises): k-means++ seeding, k-means, typicality, the rounds.
Writes one JSON (--out) and prints it.  There is no CPU fallback: without a GPU the tool fails.
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

PEAK_TFLOPS = 157.3
STEPS = ("embedding_rows", "pair_form", "typiclust")


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


def _pools(a, torch):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20)
    emb = torch.randn((a.rows, a.emb), generator=gen, device="cuda")
    n, g, D = a.pool, a.gallery, a.features
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    return {"embedding_rows": emb, "pair_form": (left, right, li, ri)}


def _stats(ms, flop):
    med = float(np.median(ms))
    return {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
            "TFLOPs": round(flop / (med * 1e-3) / 1e12, 2), "fraction_of_peak": round(flop / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 3)}


def step_knn(a, name):
    import torch
    assert torch.cuda.is_available(), "knn_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import cluster, typiclust
    from a_link_amd.batch import _pool_rows
    rows = _pools(a, torch)[name]
    L, R, li, ri, N, D, dev = _pool_rows(rows, torch)
    pair = li is not None
    K = a.k
    flop = 2.0 * N * N * D
    groups = cluster.kmeans_device(rows, a.clusters, iters=3, seed=1)["assign"]

    def materialise():
        return L if not pair else (L.index_select(0, li.long()) - R.index_select(0, ri.long())).abs()

    chunk = min(a.chunk, N)
    yard = torch.empty((N, K), dtype=torch.int64, device=dev)
    diag = torch.arange(chunk, device=dev)

    def matmul_topk(limit=None):
        X = materialise()
        norms = (X * X).sum(dim=1)
        for lo in range(0, N if limit is None else min(N, limit), chunk):
            hi = min(lo + chunk, N)
            P = torch.matmul(X[lo:hi], X.t())
            P.mul_(-2.0).add_(norms)
            P[diag[:hi - lo], diag[:hi - lo] + lo] = float("inf")
            yard[lo:hi] = torch.topk(P, K, dim=1, largest=False, sorted=True).indices

    runs = {"knn": lambda: typiclust._knn_call(rows, K, None, False, 1e-5, True),
            "knn_grouped": lambda: typiclust._knn_call(rows, K, groups, False, 1e-5, True)}
    times = {kind: [] for kind in runs}
    out = None
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for kind, fn in runs.items():
            ms, o = _call_ms(fn)
            if it:
                times[kind].append(ms)
            if kind == "knn":
                out = o
    matmul_topk(limit=chunk)                               # (warms the GEMM and topk up on one chunk)
    torch.cuda.synchronize()
    yard_ms = [_call_ms(matmul_topk)[0] for _ in range(a.yard_repeats)]
    same = (torch.sort(out[0].long(), dim=1).values == torch.sort(yard, dim=1).values).all(dim=1).double().mean().item()
    entry = {"N": N, "D": D, "K": K, "clusters": a.clusters, "repeats": a.repeats, "yardstick_repeats": a.yard_repeats, "chunk_rows": chunk,
             "knn": _stats(times["knn"], flop), "knn_grouped": _stats(times["knn_grouped"], flop),
             "matmul_topk": _stats(yard_ms, flop),
             "yardstick_spread": round(max(yard_ms) / min(yard_ms), 3),
             "fused_over_yardstick": round(float(np.median(times["knn"])) / float(np.median(yard_ms)), 3),
             "neighbour_sets_equal": round(same, 6),
             "rows_with_k_neighbours": round(float((out[2] == K).double().mean().item()), 6)}
    return entry


def step_typiclust(a):
    import torch
    assert torch.cuda.is_available(), "knn_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import typiclust
    emb = _pools(a, torch)["embedding_rows"]
    typiclust.typiclust_device(emb[:4096], [], 16, k_nn=a.k, seed=0)          # (loads every kernel)
    torch.cuda.synchronize()
    ms = []
    picks = None
    for _ in range(2):
        t0 = time.perf_counter()
        picks, info = typiclust.typiclust_device(emb, [], a.instances, k_nn=a.k, seed=0)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"N": int(emb.shape[0]), "D": int(emb.shape[1]), "n_instances": a.instances, "k_nn": a.k, "iters": 10,
            "clusters": int(info["counts"].numel()), "clusters_kept": int(len(info["order"])), "picks": int(len(picks)),
            "call_ms": [round(m, 1) for m in ms]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--emb", type=int, default=128)
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yard-repeats", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (otherwise: each step in a child of its own)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20a_knn_timing.json"))
    a = ap.parse_args(argv)
    if a.step:
        entry = step_typiclust(a) if a.step == "typiclust" else step_knn(a, a.step)
        print("KNN_TIMING_STEP " + json.dumps(entry))
        return 0
    res = {"f32_matrix_peak_TFLOPs": PEAK_TFLOPS}
    passed = [x for x in (argv if argv is not None else sys.argv[1:])]
    for step in STEPS:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + passed, timeout=a.step_timeout,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %g s: nothing more is started" % (step, a.step_timeout), file=sys.stderr)
            return 1
        text = done.stdout.decode(errors="replace")
        lines = [ln for ln in text.splitlines() if ln.startswith("KNN_TIMING_STEP ")]
        if done.returncode != 0 or not lines:
            print(text, file=sys.stderr)
            print("step %s failed (exit status %d): nothing more is started" % (step, done.returncode), file=sys.stderr)
            return 1
        res[step] = json.loads(lines[-1][len("KNN_TIMING_STEP "):])
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
