"""Time BAIT on the device (bait.hip) at the per-GPU shape of BASELINE configs[2]: 12,500 pool x 16 gallery
images = 200,000 pairs of 512 features gathered by index from the two feature tables, head 512 / 64 / 2 (F = 64 factor columns)
— beside what the library's user could do without this work, a torch composition of the same rule, and beside BADGE at the same
batch size.

    python tools/bait_timing.py [--pool 12500] [--gallery 16] [--features 512] [--picks 256 1024] [--loop-picks 64] [--repeats 9]
                                [--step-timeout 240] [--out profiles/r25a_bait_timing.json]

Without --step the tool touches no GPU itself: it runs each step — `score`, `select`, `torch_composition`, `query`, `badge` — as a
fresh child process under its own time limit (--step-timeout seconds), one after the other, stops at the first that fails or
runs out of time, and merges their JSON.  With --step NAME it runs that step in this process and prints its JSON.  Every call is
warmed up first; HIP events on the stream around whole calls; medians over --repeats, with the minimum beside them.
  score              alink_bait_scores alone on the pool's factor rows: us, FLOP/s as 4 N F^2, its share of the f32 matrix peak
  select             alink_bait_select with --loop-picks forward picks and no prune: us per pick, the update launch included
                     (the difference to `score` is the one-workgroup launch: reduce, float64 Woodbury step, A = B Phi B)
  torch_composition  the same --loop-picks picks in torch: ((f @ A) * f).sum(1) / (1 + ((f @ B) * f).sum(1)), argmax, and a
                     float64 Woodbury step with A = B Phi B per pick; `picks_differing` counts the picks that differ from
                     the library's
  query              bait.bait_device end to end (the head's EGL pass, the factor, the read-back of the factor rows, the Gram
                     matrices and the inverse on the host, over x k forward picks and the prune) for every k of --picks
  badge              badge.badge_device at the same k, the neighbouring strategy
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

PEAK_F32_MATRIX = 157.3e12
STEPS = ("score", "select", "torch_composition", "query", "badge")
TAG = "BAIT_TIMING_STEP "


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


def _workload(a, torch):
    from a_link_amd.head import DenseHead
    n, g, D = a.pool, a.gallery, a.features
    gen = torch.Generator(device="cuda")
    gen.manual_seed(25)
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    head = DenseHead(D, h1=a.h1, h2=a.h2, lr=0.1, seed=3)
    ws = head.get_weights()
    ws[4] = ws[4] * np.float32(40.0)                       # probabilities spread over (0, 1)
    head.set_weights(ws)
    return head, left, right, li, ri


def _stats(ms, flop=None, per=1):
    med = float(np.median(ms)) / per
    out = {"us": round(med * 1e3, 2), "us_min": round(float(np.min(ms)) / per * 1e3, 2)}
    if flop:
        out.update(flop=flop, flop_per_s=round(flop / (med * 1e-3), -9), share_of_f32_matrix_peak=round(flop / (med * 1e-3) / PEAK_F32_MATRIX, 4))
    return out


def _state(head, left, right, li, ri, torch):
    """the pool's factor rows, Phi, B0 = I^-1 (nothing labelled) and the packed images of A0, B0"""
    from a_link_amd import bait
    out = head.expected_gradient_length_device(left, right, li, ri, want=("probs", "emb"))
    f = bait.fisher_factor_device(out["probs"], out["emb"])
    del out
    N, F = f.shape
    phi = torch.from_numpy(bait.fisher_matrix(f.cpu().numpy().astype(np.float64), scale=1.0 / N)).cuda()
    B0 = np.eye(F)[None]
    AB = torch.from_numpy(bait.pack_ab(phi.cpu().numpy(), B0)).cuda()
    return f, phi, B0, AB


def step(a, name):
    import torch
    assert torch.cuda.is_available(), "bait_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import badge, bait
    head, left, right, li, ri = _workload(a, torch)
    N, F = li.numel(), a.h2
    res = {"shape": {"N": N, "D": a.features, "h1": a.h1, "F": F, "blocks": 1}, "repeats": a.repeats}
    if name in ("score", "select", "torch_composition"):
        f, phi, B0, AB = _state(head, left, right, li, ri, torch)
        free = torch.ones(N, dtype=torch.uint8, device="cuda")
    if name == "score":
        run = lambda: bait.bait_scores_device(f, AB, free, want_scores=False)
        times = [_call_ms(run)[0] for _ in range(1 + a.repeats)][1:]
        res["score_pass"] = _stats(times, 4.0 * N * F * F)
        res["factor_table_bytes"] = int(f.numel() * 4)
    elif name == "select":
        k = a.loop_picks

        def run():
            B, fr = torch.from_numpy(B0.copy()).cuda(), free.clone()
            return _call_ms(lambda: bait.bait_select_device(f, phi, B, fr, k, k))
        runs = [run() for _ in range(1 + a.repeats)][1:]
        res["per_pick"] = dict(_stats([r[0] for r in runs], per=k), picks=k)
        res["picks"] = runs[-1][1][0].tolist()
    elif name == "torch_composition":
        k = a.loop_picks

        def loop():
            B = torch.eye(F, dtype=torch.float64, device="cuda")
            P = phi[0]
            fr = torch.ones(N, dtype=torch.bool, device="cuda")
            picks = []
            for _ in range(k):
                A32, B32 = (B @ P @ B).float(), B.float()
                s = ((f @ A32) * f).sum(1) / (1 + ((f @ B32) * f).sum(1))
                n = torch.argmax(torch.where(fr, s, torch.full_like(s, -float("inf"))))
                picks.append(n)
                fr[n] = False
                w = B @ f[n].double()
                B = B - torch.outer(w, w) / (1 + f[n].double() @ w)
            return torch.stack(picks)
        runs = [_call_ms(loop) for _ in range(1 + min(a.repeats, 5))][1:]
        res["per_pick"] = dict(_stats([r[0] for r in runs], per=k), picks=k)
        B, fr = torch.from_numpy(B0.copy()).cuda(), free.clone()
        mine = bait.bait_select_device(f, phi, B, fr, k, k)[0]
        res["picks_differing"] = int((mine.long() != runs[-1][1]).sum())
    elif name == "query":
        for k in a.picks:
            run = lambda: bait.bait_device(head, left, right, li, ri, n_instances=k)
            runs = [_call_ms(run) for _ in range(1 + min(a.repeats, 3))][1:]
            idx = runs[-1][1][0]
            res["bait_device_k%d" % k] = dict(ms=round(float(np.median([r[0] for r in runs])), 3), ms_min=round(float(np.min([r[0] for r in runs])), 3),
                                              forward_picks=2 * k, picks=int(idx.numel()), distinct=int(idx.unique().numel()))
    else:
        for k in a.picks:
            run = lambda: badge.badge_device(head, left, right, li, ri, n_instances=k, seed=0)
            runs = [_call_ms(run) for _ in range(1 + min(a.repeats, 3))][1:]
            res["badge_device_k%d" % k] = dict(ms=round(float(np.median([r[0] for r in runs])), 3), ms_min=round(float(np.min([r[0] for r in runs])), 3))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--h1", type=int, default=512)
    ap.add_argument("--h2", type=int, default=64)
    ap.add_argument("--picks", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--loop-picks", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (otherwise: each step in a child of its own)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25a_bait_timing.json"))
    a = ap.parse_args(argv)
    if a.step:
        print(TAG + json.dumps(step(a, a.step)))
        return 0
    res = {"peak_f32_matrix_flops": PEAK_F32_MATRIX}
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
