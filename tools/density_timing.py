"""Time information density and the cold start on the device (alink_information_density, density.hip) at the per-GPU shape of
BASELINE configs[2]: 12,500 pool x 16 gallery images = 200,000 pairs of 512 features, against a reference sample of 4,096 rows
and against the pool itself (R = N: modAL's information_density, and the cold start of the ranked batch).

    python tools/density_timing.py [--pool 12500] [--gallery 16] [--features 512] [--reference 4096] [--repeats 5]
                                   [--host-rows 8192] [--no-self] [--out profiles/r16a_density_timing.json]

Both row forms on the same pool, alternating, every shape warmed up first, HIP events around whole calls (medians over --repeats):
  row form   density.information_density_device on the materialised (N, D) rows |left[li] - right[ri]|, all three outputs
  pair form  the same on (left, right, li, ri): rows formed on the fly from the two feature tables
each against the sample (a materialised (R, D) table) and against itself.  The yardstick, timed in the same walk:
batch.ranked_batch_device with --reference labelled rows and ONE pick — rb_init_kernel, the kernel this one shares its inner loop
with, plus one streaming pass.  Every time is also given as subtract / multiply-add lane operations per second (2 N R D per call)
and as a fraction of the packed-FP32 peak (256 CUs x 4 SIMDs x 16 lanes x 2 x 2.4 GHz = 7.86e13 per second).
  cold       batch.ranked_batch_cold_device for 1,024 picks on the pair form (one call, after the walk): the cold start end to end
  host       density.information_density (float64 NumPy + sklearn, the full matrix) on the first --host-rows rows, host clock;
             it cannot run at N = 200,000 (320 GB), so its time there is EXTRAPOLATED by (N / rows)^2 and named so.
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

PEAK_LANE_OPS = 256 * 4 * 16 * 2 * 2.4e9


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
    ap.add_argument("--reference", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--k", type=int, default=1024, help="picks of the one cold ranked batch (0: skip it)")
    ap.add_argument("--host-rows", type=int, default=8192, help="rows of the host form to time (0: skip it)")
    ap.add_argument("--no-self", action="store_true", help="skip R = N (seconds per call)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16a_density_timing.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "density_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd import batch as B, density as Dn

    n, g, D, R = a.pool, a.gallery, a.features, a.reference
    N = n * g
    gen = torch.Generator(device="cuda")
    gen.manual_seed(15)
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    rows = (left[li.long()] - right[ri.long()]).abs().contiguous()
    sample = rows[torch.randperm(N, generator=gen, device="cuda")[:R]].contiguous()
    utility = torch.rand(N, generator=gen, device="cuda")
    want = Dn.DEVICE_OUTPUTS

    forms = {"row_form": rows, "pair_form": (left, right, li, ri)}
    refs = {"sample": sample} if a.no_self else {"sample": sample, "self": None}
    times = {(f, r): [] for f in forms for r in refs}
    times.update({(f, "ranked_batch_init"): [] for f in forms})
    outs = {}
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for f, pool in forms.items():
            for r, ref in refs.items():
                ms, outs[f, r] = _call_ms(lambda: Dn.information_density_device(pool, ref, want=want))
                if it:
                    times[f, r].append(ms)
            ms, _ = _call_ms(lambda: B.ranked_batch_device(pool, utility, sample, 1))
            if it:
                times[f, "ranked_batch_init"].append(ms)
    same = all(torch.equal(outs["row_form", r][w], outs["pair_form", r][w]) for r in refs for w in want)
    res = {"shape": {"N": N, "D": D, "R_sample": R, "pool_images": n, "gallery_images": g}, "repeats": a.repeats,
           "peak_lane_ops_per_s": PEAK_LANE_OPS, "forms_give_the_same_bits": bool(same)}
    for (f, r), ms in times.items():
        med = float(np.median(ms))
        ops = 2.0 * N * (N if r == "self" else R) * D
        res.setdefault(f, {})[r] = {"ms_per_call": round(med, 3), "ms_per_call_min": round(float(np.min(ms)), 3), "lane_ops": ops,
                                    "lane_ops_per_s": round(ops / (med * 1e-3), -9), "fraction_of_peak": round(ops / (med * 1e-3) / PEAK_LANE_OPS, 4),
                                    "times_the_peak_time": round(med * 1e-3 * PEAK_LANE_OPS / ops, 2)}
    for f in forms:
        for r in refs:
            res[f][r]["rate_vs_ranked_batch_init"] = round(res[f][r]["lane_ops_per_s"] / res[f]["ranked_batch_init"]["lane_ops_per_s"], 3)
    last = "self" if "self" in refs else "sample"
    dens = outs["row_form", last]["density"]
    res["density_" + last] = {"min": float(dens.min()), "max": float(dens.max()), "distinct_float32_values": int(dens.unique().numel()),
                              "central": int(outs["row_form", last]["central"])}
    if a.k > 0 and not a.no_self:
        ms, (idx, _) = _call_ms(lambda: B.ranked_batch_cold_device(forms["pair_form"], utility, a.k))
        res["cold_ranked_batch_pair_form"] = {"k": a.k, "ms_per_call": round(ms, 1), "first_pick_is_central": int(idx[0]) == res["density_self"]["central"]}
    if a.host_rows > 0:
        m = min(a.host_rows, N)
        Xh = rows[:m].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        got = Dn.information_density(Xh)
        sec = time.perf_counter() - t0
        dev = Dn.information_density_device(rows[:m].contiguous())["density"].cpu().numpy()
        res["host"] = {"rows_timed": m, "s_per_call": round(sec, 3), "s_per_call_at_N_extrapolated": round(sec * (N / m) ** 2, 1),
                       "matrix_bytes_at_N": 8 * N * N, "largest_abs_difference_to_device": float(np.abs(got - dev).max())}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
