"""Time facility-location selection on the device (alink_facility_gains, alink_facility_cover, alink_facility_select, facility.hip;
a-link_amd/facility.py) beside what the library's user could do without this work — a torch composition of the same rule in the
same process on the same rows — and beside ProbCover's count pass, which shares the tile loop.

    python tools/facility_timing.py [--rows 200000] [--emb 128] [--pool 12500] [--gallery 16] [--features 512] [--kept 10240]
                                    [--k 1024] [--candidates 1024] [--repeats 7] [--batch-repeats 2] [--ball-rows 16384]
                                    [--chunk 16384] [--step-timeout 300] [--out profiles/r26a_facility_timing.json]

Without --step the tool touches no GPU itself: it runs each step — `embedding_rows`, `pair_form`, `fass` — as a fresh child process
under its own time limit (--step-timeout seconds), one after the other, stops at the first that fails or runs out of time, and
merges their JSON.  With --step NAME it runs that step in this process and prints its JSON.

Three workloads: `embedding_rows`, a (--rows, --emb) table of Gaussian rows; `pair_form`, --pool x --gallery pairs of --features
features formed on the fly from two tables of unit vectors — both with --k picks among --candidates sampled candidates per pick
(facility.sample_candidates' stream at that R); and `fass`, the --kept rows FASS keeps of the first table, every row a candidate at
every pick.  Every shape is warmed up first; HIP events on the stream around whole calls; medians over --repeats (the batches:
--batch-repeats), with the minimum and maximum beside them.
  gains          facility.gains_device with one candidate list: the norm pass, the gains pass, the sum of the slabs.  TFLOP/s =
                 2 N R D over that whole time, against the 157.3 TFLOP/s f32 matrix peak — a whole-call rate, not a kernel's.
  batch          facility.select_device with all --k picks: one norm pass and three launches per pick.  `per_pick_ms` is that
                 time over k: the full three-launch pick.
  torch_gains,   the yardstick: per chunk of --chunk pool rows xn[:, None] + cn[None, :] - 2 X @ C.T, clamp_min(0),
  torch_batch    (cur[:, None] - w).clamp_min(0).sum(0) into float64; then argmax, the pick's column and torch.minimum — nothing
                 read back.  The pair form has no row table: it is materialised once, outside the timed region (in the
                 yardstick's favour).  `gains_over_yardstick`, `batch_over_yardstick`: ours over it.  `picks_equal`,
                 `first_difference`: whether the two batches picked the same rows (the product rounds differently, and a greedy
                 that once differs keeps differing).
  ball_count     probcover.ball_count_device over the first --ball-rows rows (the whole pool costs N^2): the same tile loop with
                 a popcount epilogue.  `rate_over_ball_count` is the gains call's scores per second over its — the expectation to
                 test is about 1.
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
STEPS = ("embedding_rows", "pair_form", "fass")
TAG = "FACILITY_TIMING_STEP "


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


def _stats(ms, flop=None):
    med = float(np.median(ms))
    out = {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
    if flop is not None:
        out["TFLOPs"] = round(flop / (med * 1e-3) / 1e12, 2)
        out["fraction_of_peak"] = round(flop / (med * 1e-3) / 1e12 / PEAK_TFLOPS, 3)
    return out


def _workload(a, name, torch):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(26)
    if name == "embedding_rows":
        return torch.randn((a.rows, a.emb), generator=gen, device="cuda")
    if name == "fass":
        return torch.randn((a.rows, a.emb), generator=gen, device="cuda")[:a.kept].contiguous()
    n, g, D = a.pool, a.gallery, a.features
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    return (left, right, li, ri)


def step(a, name):
    import torch
    assert torch.cuda.is_available(), "facility_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import facility, probcover
    from a_link_amd.batch import _pool_rows
    rows = _workload(a, name, torch)
    L, Rt, li, ri, N, D, dev = _pool_rows(rows, torch)
    pair = li is not None
    k = min(a.k, N)
    X = L if not pair else (L.index_select(0, li.long()) - Rt.index_select(0, ri.long())).abs()    # the yardstick's row table
    xn = (X * X).sum(dim=1)
    cap = float(4 * xn.max())
    cur0 = torch.full((N,), cap, dtype=torch.float32, device=dev)
    if name == "fass":
        R, cand = N, None
    else:
        R = min(a.candidates, N)
        cand = torch.from_numpy(np.random.RandomState(26).randint(0, N, (k, R)).astype(np.int32)).to(dev)
    every = torch.arange(N, device=dev)
    chunk = min(a.chunk, N)

    def torch_gains(cur, c):
        C, cn = X.index_select(0, c), xn.index_select(0, c)
        g = torch.zeros(c.numel(), dtype=torch.float64, device=dev)
        for lo in range(0, N, chunk):
            w = torch.addmm(xn[lo:lo + chunk, None] + cn[None, :], X[lo:lo + chunk], C.t(), alpha=-2.0).clamp_min_(0)
            g += (cur[lo:lo + chunk, None] - w).clamp_min_(0).sum(dim=0, dtype=torch.float64)
        return g

    def torch_batch():
        cur, picks = cur0.clone(), []
        for t in range(k):
            c = every if cand is None else cand[t].long()
            p = c[torch.argmax(torch_gains(cur, c))]
            cur = torch.minimum(cur, (xn + xn[p] - 2.0 * (X @ X[p])).clamp_min_(0))
            picks.append(p)
        return torch.stack(picks)

    c0 = every if cand is None else cand[0].long()
    cur1 = facility.cover_device(rows, cur0, c0[:1].to(torch.int32))                               # a cur that is not flat
    runs = {"gains": lambda: facility.gains_device(rows, cur1, None if cand is None else cand[0]),
            "torch_gains": lambda: torch_gains(cur1, c0)}
    times = {kind: [] for kind in runs}
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for kind, fn in runs.items():
            ms, _ = _call_ms(fn)
            if it:
                times[kind].append(ms)
    batches = {"batch": lambda: facility.select_device(rows, cur0, k, cand)[0], "torch_batch": torch_batch}
    btimes, last = {kind: [] for kind in batches}, {}
    for it in range(a.batch_repeats):
        for kind, fn in batches.items():
            if kind == "torch_batch" and it:               # the yardstick's batch once: it is the long one
                continue
            ms, last[kind] = _call_ms(fn)
            btimes[kind].append(ms)
    nb = min(a.ball_rows, N)
    sub = X[:nb].contiguous() if not pair else (L, Rt, li[:nb].contiguous(), ri[:nb].contiguous())
    delta = float(torch.sqrt(xn[:nb].mean()))                                                       # (the radius does not change the work)
    ball_ms = []
    for it in range(1 + min(a.repeats, 3)):
        ms, _ = _call_ms(lambda: probcover.ball_count_device(sub, delta))
        if it:
            ball_ms.append(ms)
    ours, yard = last["batch"].long().cpu().numpy(), last["torch_batch"].cpu().numpy()
    differ = np.flatnonzero(ours != yard)
    med = {kind: float(np.median(v)) for kind, v in list(times.items()) + list(btimes.items())}
    flop = 2.0 * N * R * D
    return {"N": N, "D": D, "R": R, "k": k, "form": "pair" if pair else "rows", "repeats": a.repeats, "batch_repeats": a.batch_repeats,
            "chunk_rows": chunk, "gains": _stats(times["gains"], flop), "torch_gains": _stats(times["torch_gains"], flop),
            "batch": _stats(btimes["batch"]), "torch_batch": _stats(btimes["torch_batch"]),
            "per_pick_ms": round(med["batch"] / k, 4), "torch_per_pick_ms": round(med["torch_batch"] / k, 4),
            "gains_over_yardstick": round(med["gains"] / med["torch_gains"], 3),
            "batch_over_yardstick": round(med["batch"] / med["torch_batch"], 3),
            "picks_equal": bool(differ.size == 0), "first_difference": int(differ[0]) if differ.size else -1,
            "picks_in_common": int(len(set(ours.tolist()) & set(yard.tolist()))),
            "ball_count": dict(_stats(ball_ms, 2.0 * nb * nb * D), rows=nb),
            "rate_over_ball_count": round((float(N) * R / med["gains"]) / (float(nb) * nb / float(np.median(ball_ms))), 3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--emb", type=int, default=128)
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--kept", type=int, default=10240)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch-repeats", type=int, default=2)
    ap.add_argument("--ball-rows", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (otherwise: each step in a child of its own)")
    ap.add_argument("--step-timeout", type=float, default=300.0, help="seconds a step's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26a_facility_timing.json"))
    a = ap.parse_args(argv)
    if a.step:
        print(TAG + json.dumps(step(a, a.step)))
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
        lines = [ln for ln in text.splitlines() if ln.startswith(TAG)]
        if done.returncode != 0 or not lines:
            print(text, file=sys.stderr)
            print("step %s failed (exit status %d): nothing more is started" % (name, done.returncode), file=sys.stderr)
            return 1
        res[name] = json.loads(lines[-1][len(TAG):])
        print("step %s done" % name, file=sys.stderr, flush=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
