"""Time committee disagreement on the device (alink_committee_disagreement, select.hip) at the per-GPU shape of BASELINE
configs[2] (three members, two classes, 12,500 pool x 16 gallery images = 200,000 pairs) and at the whole job's 1,600,000 pairs.

    python tools/disagreement_profile.py [--pairs 200000 1600000] [--members 3] [--classes 2] [--repeats 200]

Per pair count, with HIP events (every shape warmed up first, medians over --repeats):
  kernel    the disagreement launch alone, for `vote_entropy`, for `max_disagreement` (which reads the members' rows twice) and
            for all five outputs: one launch between two events (includes the launch latency) and --burst launches back to back
            between two events, per launch (what a queue of them sustains); bytes per launch from the shapes, GB/s over the
            back-to-back time.  For the kernel's own duration run the tool under `rocprofv3 --kernel-trace` with --kernel-only.
  pool      members' head forwards (head.committee_member_probs_device on 512-wide embeddings through index lists) + the
            disagreement launch + uncertainty.topk_device (k = --k), the three legs and their sum.
  host      the arithmetic of learners.vote_entropy_sampling (one vote per member, the vote count loop over pairs x classes,
            multi_argmax) on the same probabilities, host clock, once.
Prints one JSON line.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUTPUTS = ("vote_entropy", "consensus_entropy", "max_disagreement", "consensus", "votes")


def bytes_per_launch(M, P, C, want):
    """what the algorithm has to move: every member's slab once, every requested output once (the second reading of the rows that
    max_disagreement makes is meant to come from cache and is not counted)"""
    out = {"vote_entropy": 4 * P, "consensus_entropy": 4 * P, "max_disagreement": 4 * P, "consensus": 4 * P * C, "votes": 4 * P * M}
    return 4 * M * P * C + sum(out[w] for w in want)


def _median_ms(fn, repeats, inner=1):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(repeats):
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / inner)
    return float(np.median(times)), float(np.min(times))


def _kernel_call(members, want):
    """the raw entry point on preallocated outputs: nothing but the launch between the events"""
    import ctypes as C
    import torch
    from a_link_amd import _abi
    lib = _abi.init(0)
    M, (P, Cn) = len(members), members[0].shape
    shapes = {"consensus": ((P, Cn), torch.float32), "votes": ((P, M), torch.int32)}
    outs = {}
    for w in want:
        shape, dtype = shapes.get(w, ((P,), torch.float32))
        outs[w] = torch.empty(shape, dtype=dtype, device="cuda")
    arr = (C.c_void_p * M)(*[t.data_ptr() for t in members])
    ptrs = [_abi.ptr(outs.get(w)) for w in OUTPUTS]
    stream = _abi.current_stream(members[0].device)

    def call():
        _abi.check(lib.alink_committee_disagreement(arr, M, P, Cn, *ptrs, stream), "alink_committee_disagreement")
    call.keep = (outs, arr)
    return call


def _member_probs(M, P, Cn, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    scale = torch.tensor([0.1, 1.0, 5.0, 30.0], device="cuda")[torch.randint(0, 4, (1, P, 1), generator=g, device="cuda")]
    return torch.softmax(torch.randn((M, P, Cn), generator=g, device="cuda") * scale, dim=2).contiguous()


def profile_kernel(a, P):
    members = list(_member_probs(a.members, P, a.classes, 1).unbind(0))
    res = {}
    for label, want in (("vote_entropy", ("vote_entropy",)), ("max_disagreement", ("max_disagreement",)), ("all_outputs", OUTPUTS)):
        call = _kernel_call(members, want)
        for _ in range(10):
            call()
        one, one_min = _median_ms(call, a.repeats)
        burst, burst_min = _median_ms(call, max(5, a.repeats // 10), inner=a.burst)
        nbytes = bytes_per_launch(a.members, P, a.classes, want)
        res[label] = {"bytes_per_launch": nbytes, "one_launch_us": round(1e3 * one, 2), "one_launch_min_us": round(1e3 * one_min, 2),
                      "back_to_back_us": round(1e3 * burst, 2), "back_to_back_min_us": round(1e3 * burst_min, 2),
                      "GBps_back_to_back": round(nbytes / (burst * 1e-3) / 1e9, 1)}
    return res


def profile_pool(a, P):
    import torch
    from a_link_amd import disagreement as D, head as H, uncertainty as U
    from a_link_amd.head import DenseHead
    g = 16
    n = P // g
    rng = np.random.RandomState(2)
    heads = []
    for m in range(a.members):
        h = DenseHead(512, lr=0.1, seed=10 + m)
        ws = h.get_weights()
        ws[4] = ws[4] * np.float32(40.0)                   # probabilities spread over (0, 1): members that do disagree
        h.set_weights(ws)
        heads.append(h)
    Ep = [torch.from_numpy(rng.randn(n, 512).astype(np.float32)).cuda() for _ in heads]
    Eg = [torch.from_numpy(rng.randn(g, 512).astype(np.float32)).cuda() for _ in heads]
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    legs = []
    for it in range(3 + a.pool_repeats):                   # the first walks warm every shape up
        ev[0].record()
        probs = H.committee_member_probs_device(heads, Ep, Eg, li, ri)
        ev[1].record()
        scores = D.score_members_device(probs, want=(a.kind,))[a.kind]
        ev[2].record()
        idx, vals = U.topk_device(scores, a.k, largest=True)
        ev[3].record()
        torch.cuda.synchronize()
        if it >= 3:
            legs.append([ev[i].elapsed_time(ev[i + 1]) for i in range(3)])
    med = np.median(np.asarray(legs), axis=0)
    res = {"kind": a.kind, "k": a.k, "pairs": n * g, "members_forward_ms": round(float(med[0]), 4), "disagreement_ms": round(float(med[1]), 4),
           "topk_ms": round(float(med[2]), 4), "total_ms": round(float(med.sum()), 4), "distinct_scores": int(torch.unique(scores).numel())}
    return res, probs.cpu().numpy()


def profile_host(probs, k):
    """learners.vote_entropy_sampling as it stands, on a committee that answers from these probabilities: what is timed is the
    sampler's own arithmetic (the members' forwards are not in it)"""
    from a_link_amd import learners

    class _Answering:
        classes_ = np.arange(probs.shape[2])

        def __len__(self):
            return probs.shape[0]

        def vote(self, X):
            return np.stack([self.classes_[np.argmax(p, axis=1)] for p in probs], axis=1).astype(np.float64)
    X = [np.zeros((probs.shape[1], 1), np.float32)] * 2
    t0 = time.perf_counter()
    idx, _ = learners.vote_entropy_sampling(_Answering(), X, n_instances=k)
    return {"vote_entropy_sampling_s": round(time.perf_counter() - t0, 3), "picked": int(len(idx))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, nargs="+", default=[200000, 1600000])
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--burst", type=int, default=50, help="launches between two events in the back-to-back form")
    ap.add_argument("--pool-repeats", type=int, default=10)
    ap.add_argument("--kind", default="vote_entropy")
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--kernel-only", action="store_true", help="the launches alone (for a run under rocprofv3 --kernel-trace)")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "disagreement_profile measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    out = {"members": a.members, "classes": a.classes, "shapes": {}}
    for P in a.pairs:
        r = {"kernel": profile_kernel(a, P)}
        if not a.kernel_only:
            if a.classes != 2:
                raise SystemExit("the pool leg runs the pair heads, which have two classes: use --kernel-only with --classes %d" % a.classes)
            r["pool"], probs = profile_pool(a, P)
            if not a.no_host:
                r["host"] = profile_host(probs, a.k)
        out["shapes"][str(P)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
