"""Time the delta-ball graph and the greedy maximum coverage on the device (alink_ball_count, alink_ball_fill, alink_max_coverage,
probcover.hip) beside alink_knn on the same rows and beside what the library's user could do without this work: torch.cdist of a
chunk of rows with the whole pool, a mask, torch.nonzero — in the same process on the same rows — and one end-to-end ProbCover call.

    python tools/probcover_timing.py [--rows 200000] [--emb 128] [--pool 12500] [--gallery 16] [--features 512] [--blobs 4096]
                                     [--spread 0.25] [--clusters 1024] [--alpha 0.95] [--picks 1024] [--k 20] [--repeats 5]
                                     [--yard-repeats 2] [--chunk 2048] [--max-edges 300000000] [--step-timeout 240]
                                     [--out profiles/r21a_probcover_timing.json]

Without --step the tool touches no GPU itself: it runs each step — `embedding_rows`, `pair_form`, `probcover` — as a fresh child
process under its own time limit (--step-timeout seconds), one after the other, stops at the first that fails or runs out of
time, and merges their JSON.  With --step NAME it runs that step in this process and prints its JSON.

Two pools: `embedding_rows`, a (--rows, --emb) row table of --blobs Gaussian blobs (unit-variance centres, rows --spread round
them: a pool with the cluster structure the purity radius presumes), and `pair_form`, --pool x --gallery pairs of --features
features formed on the fly from two tables of unit vectors.  Every shape is warmed up first; HIP events on the stream around whole
calls; the fused calls alternate inside one loop; medians over --repeats, with the minimum and maximum beside them.  delta is
probcover.purity_radius_device at --alpha over cluster.kmeans_device's --clusters clusters (3 iterations); if its graph would hold
more than --max-edges edges, radius2 is halved until it does not, and the entry says so.
  count          alink_ball_count, degrees only: the norms and the fused product + threshold.  TFLOP/s = 2 N^2 D over that whole
                 time, against the 157.3 TFLOP/s f32 matrix peak — a whole-call rate, not a kernel's.
  count_purity   the same with t_other / j_other against the k-means groups: the pass purity_radius_device makes
  graph          probcover.ball_graph_device: count, torch.cumsum, the read-back of E, the allocation, alink_ball_fill, the read-back
                 of its mismatch count
  knn            alink_knn with every output, K = --k, no groups, on the same rows in the same loop; `count_over_knn` is count over it
  cdist_nonzero  the yardstick: per chunk of --chunk rows torch.cdist(chunk, pool) into a (chunk, N) buffer, `< delta`,
                 torch.nonzero, the columns kept and the chunks concatenated at the end (no offsets are formed: LESS work than graph
                 does).  The pair form has no row table: it is materialised first, inside the timed region.
                 `graph_over_yardstick` is graph over it; `edges_yardstick` its edge count beside `edges` (cdist rounds
                 differently: pairs within rounding of the radius may differ).
  greedy         alink_max_coverage, --picks picks over that graph: two launches per pick, the E edges streamed once per pick
  probcover      (the third step) one probcover.probcover_device call on the embedding rows with delta=None and the k-means groups,
                 n_instances = --picks, nothing labelled, host clock around the call (it reads back, which synchronises): the
                 purity pass, the sort, the graph, the greedy.  The k-means before it is timed beside it.
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
STEPS = ("embedding_rows", "pair_form", "probcover")


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
    gen.manual_seed(21)
    centres = torch.randn((a.blobs, a.emb), generator=gen, device="cuda")
    member = torch.randint(0, a.blobs, (a.rows,), generator=gen, device="cuda")
    emb = centres[member] + a.spread * torch.randn((a.rows, a.emb), generator=gen, device="cuda")
    n, g, D = a.pool, a.gallery, a.features
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    return {"embedding_rows": emb.contiguous(), "pair_form": (left, right, li, ri)}


def _stats(ms, flop=None):
    med = float(np.median(ms))
    out = {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
    if flop is not None:
        out["TFLOPs"] = round(flop / (med * 1e-3) / 1e12, 2)
        out["fraction_of_peak"] = round(flop / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 3)
    return out


def _radius(a, rows, groups, probcover, torch):
    """the purity radius, halved in radius2 until the graph holds at most --max-edges edges -> (delta, edges, halvings)"""
    delta = probcover.purity_radius_device(rows, groups, a.alpha)
    halvings = 0
    while True:
        edges = int(probcover.ball_count_device(rows, delta).sum(dtype=torch.int64))
        if edges <= a.max_edges:
            return delta, edges, halvings
        delta, halvings = delta / np.sqrt(2.0), halvings + 1


def step_graph(a, name):
    import torch
    assert torch.cuda.is_available(), "probcover_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import cluster, probcover, typiclust
    from a_link_amd.batch import _pool_rows
    rows = _pools(a, torch)[name]
    L, R, li, ri, N, D, dev = _pool_rows(rows, torch)
    pair = li is not None
    flop = 2.0 * N * N * D
    groups = cluster.kmeans_device(rows, a.clusters, iters=3, seed=1)["assign"]
    delta, edges, halvings = _radius(a, rows, groups, probcover, torch)
    r2 = probcover.radius2_of(delta)
    pool = probcover._pool(rows, None, "probcover_timing")
    gpool = probcover._pool(rows, groups, "probcover_timing")

    def materialise():
        return L if not pair else (L.index_select(0, li.long()) - R.index_select(0, ri.long())).abs()

    chunk = min(a.chunk, N)

    def cdist_nonzero(limit=None):
        X = materialise()
        cols = []
        for lo in range(0, N if limit is None else min(N, limit), chunk):
            hi = min(lo + chunk, N)
            cols.append(torch.nonzero(torch.cdist(X[lo:hi], X) < delta)[:, 1].to(torch.int32))
        return torch.cat(cols)

    runs = {"count": lambda: probcover._ball_count(pool, r2, True, False),
            "count_purity": lambda: probcover._ball_count(gpool, r2, True, True),
            "graph": lambda: probcover.ball_graph_device(rows, delta),
            "knn": lambda: typiclust._knn_call(rows, a.k, None, False, 1e-5, True)}
    times = {kind: [] for kind in runs}
    graph = None
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for kind, fn in runs.items():
            ms, o = _call_ms(fn)
            if it:
                times[kind].append(ms)
            if kind == "graph":
                graph = o
    offsets, nbr = graph
    assert int(offsets[-1]) == edges == nbr.numel()
    greedy_ms, out = [], None
    for it in range(1 + min(a.repeats, 3)):
        ms, out = _call_ms(lambda: probcover.max_coverage_device(offsets, nbr, a.picks))
        if it:
            greedy_ms.append(ms)
    picks, gain, covered = out
    cdist_nonzero(limit=chunk)                             # (warms cdist and nonzero up on one chunk)
    torch.cuda.synchronize()
    yard_ms, yard_edges = [], None
    for _ in range(a.yard_repeats):
        ms, o = _call_ms(cdist_nonzero)
        yard_ms.append(ms)
        yard_edges = int(o.numel())
        del o
    deg = offsets[1:] - offsets[:-1]
    med = {kind: float(np.median(v)) for kind, v in times.items()}
    return {"N": N, "D": D, "clusters": a.clusters, "alpha": a.alpha, "delta": round(float(delta), 6), "radius2_halvings": halvings,
            "edges": edges, "mean_degree": round(edges / N, 2), "max_degree": int(deg.max()), "repeats": a.repeats,
            "yardstick_repeats": a.yard_repeats, "chunk_rows": chunk, "K_knn": a.k,
            "count": _stats(times["count"], flop), "count_purity": _stats(times["count_purity"], flop),
            "graph": _stats(times["graph"], flop), "knn": _stats(times["knn"], flop), "cdist_nonzero": _stats(yard_ms, flop),
            "count_over_knn": round(med["count"] / med["knn"], 3), "graph_over_knn": round(med["graph"] / med["knn"], 3),
            "graph_over_yardstick": round(med["graph"] / float(np.median(yard_ms)), 3),
            "yardstick_spread": round(max(yard_ms) / min(yard_ms), 3), "edges_yardstick": yard_edges,
            "greedy": dict(_stats(greedy_ms), picks=a.picks, real_picks=int((picks >= 0).sum()), first_gain=int(gain[0]),
                           covered_share=round(float(covered.double().mean()), 6),
                           ms_per_pick=round(float(np.median(greedy_ms)) / a.picks, 4))}


def step_probcover(a):
    import torch
    assert torch.cuda.is_available(), "probcover_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import cluster, probcover
    emb = _pools(a, torch)["embedding_rows"]
    small = emb[:4096].contiguous()
    g = cluster.kmeans_device(small, 16, iters=1, seed=0)["assign"]
    probcover.probcover_device(small, [], 16, groups=g, alpha=a.alpha)     # (loads every kernel)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    groups = cluster.kmeans_device(emb, a.clusters, iters=3, seed=1)["assign"]
    torch.cuda.synchronize()
    kmeans_ms = (time.perf_counter() - t0) * 1e3
    ms, picks, info = [], None, None
    for _ in range(2):
        t0 = time.perf_counter()
        picks, info = probcover.probcover_device(emb, [], a.picks, groups=groups, alpha=a.alpha)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"N": int(emb.shape[0]), "D": int(emb.shape[1]), "n_instances": a.picks, "clusters": a.clusters, "alpha": a.alpha,
            "kmeans_ms": round(kmeans_ms, 1), "delta": round(info["delta"], 6), "edges": info["edges"], "picks": int(len(picks)),
            "covered": round(info["covered"], 6), "exhausted": info["exhausted"], "call_ms": [round(m, 1) for m in ms]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--emb", type=int, default=128)
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--blobs", type=int, default=4096)
    ap.add_argument("--spread", type=float, default=0.25)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--alpha", type=float, default=0.95)
    ap.add_argument("--picks", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yard-repeats", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=2048)
    ap.add_argument("--max-edges", type=int, default=300000000)
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (otherwise: each step in a child of its own)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21a_probcover_timing.json"))
    a = ap.parse_args(argv)
    if a.step:
        entry = step_probcover(a) if a.step == "probcover" else step_graph(a, a.step)
        print("PROBCOVER_TIMING_STEP " + json.dumps(entry))
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
        lines = [ln for ln in text.splitlines() if ln.startswith("PROBCOVER_TIMING_STEP ")]
        if done.returncode != 0 or not lines:
            print(text, file=sys.stderr)
            print("step %s failed (exit status %d): nothing more is started" % (step, done.returncode), file=sys.stderr)
            return 1
        res[step] = json.loads(lines[-1][len("PROBCOVER_TIMING_STEP "):])
        print("step %s done" % step, file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
