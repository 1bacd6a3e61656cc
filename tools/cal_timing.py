"""Time the rectangular k-nearest-neighbour search and Contrastive Active Learning on the device (alink_knn_rect, alink_cal_score,
knn_rect.hip; a-link_amd/cal.py) beside alink_knn on the same query rows and beside what the library's user could do without this
work: torch.matmul of a chunk of materialised rows with the reference rows, the norms added, torch.topk — in the same process on
the same rows.

    python tools/cal_timing.py [--rows 200000] [--emb 128] [--pool 12500] [--gallery 16] [--features 512] [--labelled 4096]
                               [--k 10] [--classes 2] [--picks 1024] [--repeats 7] [--square-repeats 3] [--chunk 16384]
                               [--step-timeout 240] [--out profiles/r22a_cal_timing.json]

Without --step the tool touches no GPU itself: it runs each step — `embedding_rows`, `pair_form` — as a fresh child process under
its own time limit (--step-timeout seconds), one after the other, stops at the first that fails or runs out of time, and merges
their JSON.  With --step NAME it runs that step in this process and prints its JSON.

Two workloads: `embedding_rows`, a (--rows, --emb) table of Gaussian rows searched against a (--labelled, --emb) table, and
`pair_form`, --pool x --gallery pairs of --features features formed on the fly from two tables of unit vectors, searched against
--labelled of those pairs (their own index vectors into the same tables).  Every shape is warmed up first; HIP events on the
stream around whole calls; the fused calls alternate inside one loop; medians over --repeats, with the minimum and maximum
beside them.
  knn_rect       alink_knn_rect with every output (idx, d2, found), K = --k: the two norm passes, the fused product + lists, the
                 winners' distances.  TFLOP/s = 2 N M D over that whole time, against the 157.3 TFLOP/s f32 matrix peak — a
                 whole-call rate, not a kernel's.
  cal            cal.cal_device end to end with given probabilities (--classes columns): knn_rect, alink_cal_score, the top
                 --picks by uncertainty.topk_device.  In the pair form it includes cal_device's range check of li / ri, which
                 reads back.
  matmul_topk    the yardstick: per chunk of --chunk queries cn[None, :] - 2 chunk @ references.T into a (chunk, M) buffer and
                 torch.topk(k, largest=False) of it, the chunks concatenated; indices only, no distances (LESS work than knn_rect
                 does).  The pair form has no row tables: both are materialised first, inside the timed region.
                 `knn_rect_over_yardstick` is knn_rect over it; `sets_differing_from_yardstick` counts the queries whose
                 neighbour SET differs (the product rounds differently: references within rounding of the k-th may differ).
  knn            alink_knn with every output, K = --k, no groups, on the query rows themselves (--square-repeats calls):
                 TFLOP/s = 2 N^2 D.  `rate_over_knn` is knn_rect's rate per score over it — the expectation to test is about 1:
                 a workgroup's inner loop is the same.
Writes one JSON (--out) and prints it.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3
STEPS = ("embedding_rows", "pair_form")


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


def _workload(a, name, torch):
    """-> (queries, references) as knn_rect_device takes them"""
    gen = torch.Generator(device="cuda")
    gen.manual_seed(22)
    if name == "embedding_rows":
        return (torch.randn((a.rows, a.emb), generator=gen, device="cuda"), torch.randn((a.labelled, a.emb), generator=gen, device="cuda"))
    n, g, D = a.pool, a.gallery, a.features
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    lab = torch.randperm(n * g, generator=gen, device="cuda")[:a.labelled]
    return (left, right, li, ri), (left, right, li.index_select(0, lab), ri.index_select(0, lab))


def _stats(ms, flop=None):
    med = float(np.median(ms))
    out = {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
    if flop is not None:
        out["TFLOPs"] = round(flop / (med * 1e-3) / 1e12, 2)
        out["fraction_of_peak"] = round(flop / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 3)
    return out


def step(a, name):
    import torch
    assert torch.cuda.is_available(), "cal_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import cal, typiclust
    from a_link_amd.batch import _pool_rows
    queries, references = _workload(a, name, torch)
    L, R, li, ri, N, D, dev = _pool_rows(queries, torch)
    cL, cR, cli, cri, M = _pool_rows(references, torch)[:5]
    pair = li is not None
    gen = torch.Generator(device="cuda")
    gen.manual_seed(23)
    p_pool = torch.softmax(2 * torch.randn((N, a.classes), generator=gen, device="cuda"), dim=1)
    p_lab = torch.softmax(2 * torch.randn((M, a.classes), generator=gen, device="cuda"), dim=1)

    def materialise(left, right, i, j):
        return left if not pair else (left.index_select(0, i.long()) - right.index_select(0, j.long())).abs()

    chunk = min(a.chunk, N)

    def matmul_topk(limit=None):
        X, Cm = materialise(L, R, li, ri), materialise(cL, cR, cli, cri)
        cn = (Cm * Cm).sum(dim=1)
        out = []
        for lo in range(0, N if limit is None else min(N, limit), chunk):
            out.append(torch.topk(torch.addmm(cn.expand(min(lo + chunk, N) - lo, M), X[lo:lo + chunk], Cm.t(), alpha=-2.0), min(a.k, M),
                                  dim=1, largest=False).indices)
        return torch.cat(out)

    runs = {"knn_rect": lambda: cal.knn_rect_device(queries, references, a.k),
            "cal": lambda: cal.cal_device(queries, references, p_pool, p_lab, a.picks, k_nn=a.k),
            "matmul_topk": matmul_topk}
    times = {kind: [] for kind in runs}
    last = {}
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for kind, fn in runs.items():
            ms, last[kind] = _call_ms(fn)
            if it:
                times[kind].append(ms)
    square_ms = []
    for it in range(1 + a.square_repeats):
        ms, _ = _call_ms(lambda: typiclust._knn_call(queries, a.k, None, False, 1e-5, True))
        if it:
            square_ms.append(ms)
    ours = torch.sort(last["knn_rect"][0].long(), dim=1).values
    yard = torch.sort(last["matmul_topk"], dim=1).values
    med = {kind: float(np.median(v)) for kind, v in times.items()}
    rect_flop, square_flop = 2.0 * N * M * D, 2.0 * N * N * D
    rect_rate, square_rate = rect_flop / med["knn_rect"], square_flop / float(np.median(square_ms))
    return {"N": N, "M": M, "D": D, "K": a.k, "classes": a.classes, "picks": a.picks, "form": "pair" if pair else "rows",
            "repeats": a.repeats, "square_repeats": a.square_repeats, "chunk_rows": chunk,
            "knn_rect": _stats(times["knn_rect"], rect_flop), "cal": _stats(times["cal"]),
            "matmul_topk": _stats(times["matmul_topk"], rect_flop), "knn": _stats(square_ms, square_flop),
            "knn_rect_over_yardstick": round(med["knn_rect"] / med["matmul_topk"], 3),
            "cal_over_knn_rect": round(med["cal"] / med["knn_rect"], 3),
            "rate_over_knn": round(rect_rate / square_rate, 3),
            "sets_differing_from_yardstick": int((ours != yard).any(dim=1).sum()),
            "found_all": bool((last["knn_rect"][2] == min(a.k, M)).all())}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--emb", type=int, default=128)
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--labelled", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--picks", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--square-repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (otherwise: each step in a child of its own)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22a_cal_timing.json"))
    a = ap.parse_args(argv)
    if a.step:
        print("CAL_TIMING_STEP " + json.dumps(step(a, a.step)))
        return 0
    res = {"f32_matrix_peak_TFLOPs": PEAK_TFLOPS}
    passed = [x for x in (argv if argv is not None else sys.argv[1:])]
    for name in STEPS:
        try:
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name] + passed, timeout=a.step_timeout,
                                  stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        except subprocess.TimeoutExpired:
            print("step %s ran out of its %g s: nothing more is started" % (name, a.step_timeout), file=sys.stderr)
            return 1
        text = done.stdout.decode(errors="replace")
        lines = [ln for ln in text.splitlines() if ln.startswith("CAL_TIMING_STEP ")]
        if done.returncode != 0 or not lines:
            print(text, file=sys.stderr)
            print("step %s failed (exit status %d): nothing more is started" % (name, done.returncode), file=sys.stderr)
            return 1
        res[name] = json.loads(lines[-1][len("CAL_TIMING_STEP "):])
        print("step %s done" % name, file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
