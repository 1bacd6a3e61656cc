"""Time Lloyd's k-means on the device (alink_kmeans, kmeans.hip) beside what the library could do without it: the exact-f32 GEMM
(alink_gemm32_ex) forming the products of the rows with the centres in row chunks that fit, plus torch.argmin over each chunk —
in the same process on the same rows.

    python tools/kmeans_timing.py [--rows 200000] [--emb 128] [--pool 12500] [--gallery 16] [--features 512] [--k 1024]
                                  [--iters 10] [--repeats 9] [--chunk 100000] [--host-rows 8192]
                                  [--out profiles/r19a_kmeans_timing.json]

Two pools: `embedding_rows`, a (--rows, --emb) row table, and `pair_form`, --pool x --gallery pairs of --features features formed
on the fly from the two feature tables.  Centres: the first --k rows.  Every shape is warmed up first; HIP events on the stream
around whole calls; the kinds alternate inside one loop; medians over --repeats, with the minimum and maximum beside them.
  assign_pass   alink_kmeans(iters = 0) without counts / wsum / nearest: the centre norms, the fused product + argmin, the distance
                pass (d2, changed, inertia) and its reduction — one assignment as a call makes it.  TFLOP/s = 2 N K D over that
                whole time, against the 157.3 TFLOP/s f32 matrix peak.
  iteration     (alink_kmeans(iters = --iters) - alink_kmeans(iters = 0), both with every output) / --iters: one assignment and one
                update.  update = iteration - assign_pass; its bytes: the rows once (both tables' rows per pair and the index vectors
                in the pair form), the float64 partial sums written and read, and the assignment vector once per scanning wave
                (K x ceil(D / 256) waves read all N entries) — the last named apart as `scan_bytes`, it is what the form costs.
  gemm_argmin   the yardstick: per chunk of --chunk rows alink_gemm32_ex (A = the rows, B = the centres as [K][D]) into a
                (chunk, K) buffer, then scores = |c|^2 - 2 P in place and torch.argmin.  It produces the assignment only — no d2, no
                inertia — so assign_pass is compared with LESS work than it does.  The pair form has no row table to hand the
                GEMM: its chunks are materialised first (|left[li] - right[ri]| by torch), inside the timed region.  The GEMM entry
                synchronises the host after its launch (it is a test entry): the events then also see the idle gap before the next
                launch, once per chunk; --chunk is large so that there are two of them.
  `fused_over_yardstick` is assign_pass over gemm_argmin; `yardstick_spread` is max / min of the yardstick's own repeats, the
  measure of whether the ratio says anything.
  host   cluster.kmeans (float64 NumPy) on the first --host-rows embedding rows, host clock: (kmeans(iters = 3) - kmeans(iters = 1)) / 2,
         one iteration; an iteration at --rows is EXTRAPOLATED from it by the row count and named so.
Writes one JSON (--out) and prints it.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3


def _unit(t):
    return t / t.norm(dim=1, keepdim=True)


def _slices(N, K):
    """the slices the update's scan cuts the rows into (pool_tile.h: pt_slices)"""
    S = 1 if K >= 2048 else min(64, -(-4096 // K))
    L = -(-(-(-N // S)) // 256) * 256
    return -(-N // L)


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--chunk", type=int, default=100000)
    ap.add_argument("--host-rows", type=int, default=8192, help="rows of the host form to time (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19a_kmeans_timing.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "kmeans_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import _abi, cluster, net_host
    from a_link_amd.batch import _pool_rows

    lib = _abi.init(0)
    K, T = a.k, a.iters
    gen = torch.Generator(device="cuda")
    gen.manual_seed(19)
    emb = torch.randn((a.rows, a.emb), generator=gen, device="cuda")
    n, g, D = a.pool, a.gallery, a.features
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    pools = {"embedding_rows": emb, "pair_form": (left, right, li, ri)}
    res = {"K": K, "iters": T, "repeats": a.repeats, "chunk_rows": a.chunk, "f32_matrix_peak_TFLOPs": PEAK_TFLOPS}
    st = lambda: _abi.current_stream(torch.device("cuda", 0))

    for name, rows in pools.items():
        L, R, li_, ri_, N, Dn, dev = _pool_rows(rows, torch)
        pair = li_ is not None

        def materialise(lo, hi):
            return L[lo:hi] if not pair else (L.index_select(0, li_[lo:hi].long()) - R.index_select(0, ri_[lo:hi].long())).abs()
        C0 = materialise(0, K).contiguous().clone()
        scratch, sp, _ = net_host.aligned_scratch(lib.alink_kmeans_scratch_bytes(N, Dn, K), dev)
        o = {"assign": torch.empty(N, dtype=torch.int32, device=dev), "d2": torch.empty(N, dtype=torch.float32, device=dev),
             "inertia": torch.empty(T + 1, dtype=torch.float64, device=dev), "changed": torch.empty(T + 1, dtype=torch.int32, device=dev),
             "counts": torch.empty(K, dtype=torch.int32, device=dev), "wsum": torch.empty(K, dtype=torch.float64, device=dev),
             "nearest": torch.empty(K, dtype=torch.int32, device=dev)}
        cen = torch.empty_like(C0)

        def kmeans_call(iters, stats):
            cen.copy_(C0)
            s = [o[k] if stats else None for k in ("counts", "wsum", "nearest")]
            _abi.check(lib.alink_kmeans(_abi.ptr(L), _abi.ptr(R), _abi.ptr(li_), _abi.ptr(ri_), N, Dn, None, _abi.ptr(cen), K, iters,
                                        _abi.ptr(o["assign"]), _abi.ptr(o["d2"]), _abi.ptr(o["inertia"]), _abi.ptr(o["changed"]),
                                        _abi.ptr(s[0]), _abi.ptr(s[1]), _abi.ptr(s[2]), sp, st()), "alink_kmeans")

        chunk = min(a.chunk, N)
        prod = torch.empty((chunk, K), dtype=torch.float32, device=dev)
        yard = torch.empty(N, dtype=torch.int64, device=dev)
        cn = (C0.double() ** 2).sum(dim=1).float()
        ws = torch.empty(64, dtype=torch.float32, device=dev)

        def gemm_argmin():
            for lo in range(0, N, chunk):
                hi = min(lo + chunk, N)
                A = materialise(lo, hi).contiguous()
                d = _abi.Gemm32Desc()
                d.A, d.B, d.C = A.data_ptr(), C0.data_ptr(), prod.data_ptr()
                d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.amode, d.bmode = hi - lo, K, Dn, Dn, Dn, K, 0, 1
                d.splitk, d.kper = 1, 0
                _abi.check(lib.alink_gemm32_ex(C.byref(d), 1, _abi.ptr(ws), 64, None, st()), "alink_gemm32_ex")
                P = prod[:hi - lo]
                P.mul_(-2.0).add_(cn)
                torch.argmin(P, dim=1, out=yard[lo:hi])

        runs = {"assign_pass": lambda: kmeans_call(0, False), "assign_stats": lambda: kmeans_call(0, True),
                "iterations": lambda: kmeans_call(T, True), "gemm_argmin": gemm_argmin}
        times = {kind: [] for kind in runs}
        agree = None
        for it in range(1 + a.repeats):                    # the first walk warms every kernel up
            for kind, fn in runs.items():
                ms, _ = _call_ms(fn)
                if it:
                    times[kind].append(ms)
                elif kind == "gemm_argmin":
                    kmeans_call(0, False)
                    agree = float((o["assign"].long() == yard).double().mean().item())
        med = {k: float(np.median(v)) for k, v in times.items()}
        assign_ms = med["assign_pass"]
        iter_ms = (med["iterations"] - med["assign_stats"]) / T
        update_ms = iter_ms - assign_ms
        S = _slices(N, K)
        row_bytes = (2 * 4 * N * Dn + 2 * 4 * N) if pair else 4 * N * Dn
        sums_bytes = 2 * 8 * K * S * Dn
        scan_bytes = 4 * N * K * (-(-Dn // 256))
        entry = {"N": N, "D": Dn, "slices": S,
                 "assign_pass_ms": round(assign_ms, 3), "assign_pass_ms_min": round(min(times["assign_pass"]), 3),
                 "assign_pass_ms_max": round(max(times["assign_pass"]), 3),
                 "assign_TFLOPs": round(2.0 * N * K * Dn / (assign_ms * 1e-3) / 1e12, 2),
                 "assign_fraction_of_peak": round(2.0 * N * K * Dn / (assign_ms * 1e-3) / 1e12 / PEAK_TFLOPS, 3),
                 "call_ms_at_iters": round(med["iterations"], 3), "call_ms_at_0_iters": round(med["assign_stats"], 3),
                 "iteration_ms": round(iter_ms, 3), "update_ms": round(update_ms, 3),
                 "update_row_and_sum_bytes": row_bytes + sums_bytes, "update_scan_bytes": scan_bytes,
                 "update_TBps_rows_and_sums": round((row_bytes + sums_bytes) / (update_ms * 1e-3) / 1e12, 3),
                 "update_TBps_with_scan": round((row_bytes + sums_bytes + scan_bytes) / (update_ms * 1e-3) / 1e12, 3),
                 "gemm_argmin_ms": round(med["gemm_argmin"], 3), "gemm_argmin_ms_min": round(min(times["gemm_argmin"]), 3),
                 "gemm_argmin_ms_max": round(max(times["gemm_argmin"]), 3),
                 "yardstick_spread": round(max(times["gemm_argmin"]) / min(times["gemm_argmin"]), 3),
                 "fused_over_yardstick": round(assign_ms / med["gemm_argmin"], 3),
                 "rows_assigned_as_the_yardstick_does": round(agree, 6),
                 "changed": o["changed"].cpu().tolist()}
        res[name] = entry
        del prod, yard, scratch
    if a.host_rows > 0:
        hr = min(a.host_rows, a.rows)
        Xh = emb[:hr].cpu().numpy()
        Ch = emb[:K].cpu().numpy()
        cluster.kmeans(Xh, Ch, 0)                          # (warms NumPy's threads up)
        t0 = time.perf_counter()
        cluster.kmeans(Xh, Ch, 1)
        t1 = time.perf_counter()
        cluster.kmeans(Xh, Ch, 3)
        t2 = time.perf_counter()
        per_iter = ((t2 - t1) - (t1 - t0)) / 2.0
        res["host"] = {"rows": hr, "D": a.emb, "K": K, "s_per_iteration": round(per_iter, 3),
                       "s_per_iteration_extrapolated": round(per_iter * a.rows / float(hr), 1), "extrapolated_to": {"N": a.rows, "K": K}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
