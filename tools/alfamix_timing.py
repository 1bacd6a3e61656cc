"""Time ALFA-Mix's feature mix on the device (alink_head_feature_mix, alfamix.hip) at the per-GPU shape of BASELINE configs[2]:
12,500 pool x 16 gallery images = 200,000 pairs of 512 features gathered by index from the two feature tables, head 512 / 64 / 2,
A = 2 anchors — beside alink_head_forward and alink_head_egl on the same inputs, and beside what the library's user could do
without this work: a torch composition (forward, autograd input gradient, mix, one forward per anchor, in chunks).

    python tools/alfamix_timing.py [--pool 12500] [--gallery 16] [--features 512] [--anchors 2] [--eps 0.2] [--repeats 9]
                                   [--chunk 16384] [--picks 256] [--step-timeout 240] [--out profiles/r24a_alfamix_timing.json]

Without --step the tool touches no GPU itself: it runs each step — `library`, `torch_composition`, `query` — as a fresh child
process under its own time limit (--step-timeout seconds), one after the other, stops at the first that fails or runs out of
time, and merges their JSON.  With --step NAME it runs that step in this process and prints its JSON.  Every call is warmed up
first; HIP events on the stream around whole calls; the library calls alternate inside one loop; medians over --repeats, with
the minimum beside them.
  library            forward: alink_head_forward, the yardstick (it shares the dominant GEMM and its staging); egl:
                     alink_head_egl, EGL only; mix: alink_head_feature_mix, probabilities and flip masks (what a query needs);
                     mix_all: the same with the mixed probabilities and the P x A x D mixed rows written out.  By operation
                     count mix / forward is about 2 + A (the forward, the back-projection through W1 — the forward's dominant
                     GEMM transposed — and one forward per anchor).
  torch_composition  per chunk of --chunk pairs: gather |l - r|, the head in torch with autograd for the input gradient of the
                     predicted class's negative margin, the mix per anchor, the head again on every mixed row; flip masks only.
                     `flips_differing` counts the pairs whose mask differs from the library's (sums are ordered differently).
  query              alfamix.alfamix_device end to end: the mix, the candidates read off the mask, k-means over them with
                     K = --picks (10 iterations), the fill.
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
STEPS = ("library", "torch_composition", "query")
TAG = "ALFAMIX_TIMING_STEP "


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
    gen.manual_seed(24)
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    head = DenseHead(D, h1=a.h1, h2=a.h2, lr=0.1, seed=3)
    ws = head.get_weights()
    ws[4] = ws[4] * np.float32(40.0)                       # probabilities spread over (0, 1)
    head.set_weights(ws)
    # anchors: the mean rows of 2,048 pairs split by the head's own prediction, then further random pairs' rows
    lab = torch.randperm(n * g, generator=gen, device="cuda")[:2048]
    rows = (left[li[lab].long()] - right[ri[lab].long()]).abs()
    yhat = head.predict_device(rows, torch.zeros_like(rows))[:, 1] > 0.5
    means = [rows[m].double().mean(dim=0).float() if bool(m.any()) else rows.double().mean(dim=0).float() for m in (~yhat, yhat)]
    anchors = torch.stack((means + [rows[i] for i in range(8)])[:a.anchors]).contiguous()
    return head, left, right, li, ri, anchors


def _stats(ms, flop=None):
    med = float(np.median(ms))
    out = {"ms_per_call": round(med, 4), "ms_per_call_min": round(float(np.min(ms)), 4)}
    if flop:
        out.update(flop=flop, flop_per_s=round(flop / (med * 1e-3), -9), share_of_f32_matrix_peak=round(flop / (med * 1e-3) / PEAK_F32_MATRIX, 4))
    return out


def _torch_flips(ws, left, right, li, ri, anchors, eps, chunk, torch):
    W1, b1, W2, b2, W3, b3 = ws
    fwd = lambda x: torch.relu(torch.relu(x @ W1 + b1) @ W2 + b2) @ W3 + b3
    out = []
    for lo in range(0, li.numel(), chunk):
        d = (left[li[lo:lo + chunk].long()] - right[ri[lo:lo + chunk].long()]).abs().requires_grad_(True)
        z3 = fwd(d)
        yhat = z3[:, 1] > z3[:, 0]
        margin = torch.where(yhat, z3[:, 1] - z3[:, 0], z3[:, 0] - z3[:, 1])
        g, = torch.autograd.grad((-margin).sum(), d)
        d = d.detach()
        G = g.norm(dim=1)
        flip = torch.zeros(d.shape[0], dtype=torch.uint8, device=d.device)
        for k in range(anchors.shape[0]):
            z = anchors[k][None, :] - d
            t = (eps * z.norm(dim=1) / G)[:, None] * g
            delta = torch.minimum(torch.maximum(t, z.clamp(max=0)), z.clamp(min=0))
            delta = torch.where((G > 0)[:, None], delta, torch.zeros_like(delta))
            m3 = fwd(d + delta)
            flip |= ((m3[:, 1] > m3[:, 0]) != yhat).to(torch.uint8) << k
        out.append(flip)
    return torch.cat(out)


def step(a, name):
    import torch
    assert torch.cuda.is_available(), "alfamix_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import _abi, alfamix
    head, left, right, li, ri, anchors = _workload(a, torch)
    P, D, A, od = li.numel(), a.features, anchors.shape[0], 2
    res = {"shape": {"P": P, "D": D, "h1": a.h1, "h2": a.h2, "out_dim": od, "anchors": A, "eps": a.eps}, "repeats": a.repeats}
    lib, st = head.lib, _abi.current_stream(head.device)
    tables = [_abi.ptr(t) for t in (left, right, li, ri)]
    probs, flip = torch.empty((P, od), device="cuda"), torch.empty(P, dtype=torch.uint8, device="cuda")

    def mix_call(p, f, mp=None, mx=None):
        return lambda: _abi.check(lib.alink_head_feature_mix(head.h, *tables, P, _abi.ptr(anchors), A, a.eps, _abi.ptr(p), _abi.ptr(f),
                                                             _abi.ptr(mp), _abi.ptr(mx), st), "alink_head_feature_mix")
    if name == "library":
        # the library's entries themselves, on outputs allocated once (the Python entries range-check li / ri: a read-back)
        fwd, egl = torch.empty((P, od), device="cuda"), torch.empty(P, device="cuda")
        p2, f2 = torch.empty_like(probs), torch.empty_like(flip)
        mp, mx = torch.empty((P, A, od), device="cuda"), torch.empty((P, A, D), device="cuda")
        calls = {"forward": lambda: _abi.check(lib.alink_head_forward(head.h, *tables, P, _abi.ptr(fwd), st), "alink_head_forward"),
                 "egl": lambda: _abi.check(lib.alink_head_egl(head.h, *tables, P, 0, 0.0, _abi.ptr(egl), None, None, st), "alink_head_egl"),
                 "mix": mix_call(probs, flip), "mix_all": mix_call(p2, f2, mp, mx)}
        times = {k: [] for k in calls}
        for it in range(1 + a.repeats):                    # the first walk warms every kernel up
            for k, fn in calls.items():
                ms, _ = _call_ms(fn)
                if it:
                    times[k].append(ms)
        f_fwd = 2.0 * P * (D * a.h1 + a.h1 * a.h2)
        flops = {"forward": f_fwd, "egl": 2.0 * P * (D * a.h1 + 2 * a.h1 * a.h2)}
        flops["mix"] = flops["mix_all"] = (1 + A) * f_fwd + 2.0 * P * (a.h1 * a.h2 + D * a.h1)
        for k, ms in times.items():
            res[k] = _stats(ms, flops[k])
        for k in ("egl", "mix", "mix_all"):
            res[k + "_over_forward"] = round(res[k]["ms_per_call"] / res["forward"]["ms_per_call"], 3)
        res["mix_over_forward_by_operation_count"] = round(flops["mix"] / f_fwd, 3)
        res["probabilities_equal_the_forwards_bits"] = bool(torch.equal(probs, fwd))
        res["flags_alone_equal_flags_of_all_bits"] = bool(torch.equal(flip, f2))
        res["pairs_flipping_under_some_anchor"] = int((flip != 0).sum())
        res["mixed_bytes_written_by_mix_all"] = int(mx.numel() * 4)
    elif name == "torch_composition":
        ws = [torch.from_numpy(np.array(w)).cuda() for w in head.get_weights()]
        run = lambda: _torch_flips(ws, left, right, li, ri, anchors, a.eps, a.chunk, torch)
        times = []
        for it in range(1 + a.repeats):
            ms, tflip = _call_ms(run)
            if it:
                times.append(ms)
        mix_call(probs, flip)()
        ms_lib = [_call_ms(mix_call(probs, flip))[0] for _ in range(a.repeats)]
        res["torch_composition"] = dict(_stats(times), chunk=a.chunk)
        res["mix"] = _stats(ms_lib)
        res["mix_over_torch_composition"] = round(res["mix"]["ms_per_call"] / res["torch_composition"]["ms_per_call"], 3)
        res["flips_differing"] = int((tflip != flip).sum())
    else:
        run = lambda: alfamix.alfamix_device(head, left, right, li, ri, anchors, a.picks, eps=a.eps, iters=10, seed=0)
        times = []
        for it in range(1 + min(a.repeats, 3)):
            ms, (picks, info) = _call_ms(run)
            if it:
                times.append(ms)
        res["alfamix_device"] = dict(_stats(times), picks=int(picks.numel()), distinct=int(picks.unique().numel()),
                                     candidates=int((info["flip"] != 0).sum()), kmeans_iters=10)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pool", type=int, default=12500)
    ap.add_argument("--gallery", type=int, default=16)
    ap.add_argument("--features", type=int, default=512)
    ap.add_argument("--h1", type=int, default=512)
    ap.add_argument("--h2", type=int, default=64)
    ap.add_argument("--anchors", type=int, default=2)
    ap.add_argument("--eps", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--picks", type=int, default=256)
    ap.add_argument("--step", choices=STEPS, help="run this one step in this process (otherwise: each step in a child of its own)")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds a step's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24a_alfamix_timing.json"))
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
