"""Time the expected gradient length on the device (alink_head_egl, egl.hip) at the per-GPU shape of BASELINE configs[2]:
12,500 pool x 16 gallery images = 200,000 pairs of 512 features gathered by index from the two feature tables, head 512 / 64 / 2.

    python tools/egl_timing.py [--pool 12500] [--gallery 16] [--features 512] [--repeats 9] [--out profiles/r17a_egl_timing.json]

Three library calls on the same inputs and on outputs allocated once, in the same walk, alternating, every one warmed up first,
HIP events around whole calls (medians over --repeats):
  forward    alink_head_forward — the yardstick: it shares the dominant GEMM and its staging
  egl        alink_head_egl, EGL only
  egl_all    alink_head_egl, EGL + probabilities + gradient embeddings (200,000 x 128 floats more to write)
Every time is also given as FLOP/s from 2 (D h1 + h1 h2) per pair for the forward and 2 (D h1 + 2 h1 h2) for the EGL (its
third GEMM), and as a share of the f32 matrix peak (157.3 TF).  By operation count egl / forward is
(D h1 + 2 h1 h2) / (D h1 + h1 h2) = 1.11 at this shape, plus the epilogue.
Writes one JSON (--out) and prints it.  There is no CPU fallback: without a GPU the tool fails.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX = 157.3e12


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
    ap.add_argument("--h1", type=int, default=512)
    ap.add_argument("--h2", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17a_egl_timing.json"))
    a = ap.parse_args(argv)
    import torch
    assert torch.cuda.is_available(), "egl_timing measures on the GPU: there is nothing to time without one"
    import a_link_amd  # noqa: F401
    from a_link_amd.head import DenseHead

    n, g, D = a.pool, a.gallery, a.features
    P = n * g
    gen = torch.Generator(device="cuda")
    gen.manual_seed(17)
    left = _unit(torch.randn((n, D), generator=gen, device="cuda"))
    right = _unit(torch.randn((g, D), generator=gen, device="cuda"))
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    head = DenseHead(D, h1=a.h1, h2=a.h2, lr=0.1, seed=3)
    ws = head.get_weights()
    ws[4] = ws[4] * np.float32(40.0)                       # probabilities spread over (0, 1)
    head.set_weights(ws)
    # the library's entries themselves, on outputs allocated once: the Python entry of the EGL range-checks li / ri (a read-back),
    # DenseHead.predict_device does not, and neither belongs in a comparison of the two launches
    from a_link_amd import _abi
    lib, st = head.lib, _abi.current_stream(head.device)
    fwd = torch.empty((P, 2), dtype=torch.float32, device="cuda")
    outs = {"forward": fwd, "egl": {"egl": torch.empty(P, device="cuda")},
            "egl_all": {"egl": torch.empty(P, device="cuda"), "probs": torch.empty((P, 2), device="cuda"), "emb": torch.empty((P, 2 * a.h2), device="cuda")}}
    tables = [_abi.ptr(t) for t in (left, right, li, ri)]

    def egl_call(o):
        return lambda: _abi.check(lib.alink_head_egl(head.h, *tables, P, 0, 0.0, _abi.ptr(o["egl"]), _abi.ptr(o.get("probs")), _abi.ptr(o.get("emb")), st),
                                  "alink_head_egl")
    calls = {"forward": lambda: _abi.check(lib.alink_head_forward(head.h, *tables, P, _abi.ptr(fwd), st), "alink_head_forward"),
             "egl": egl_call(outs["egl"]), "egl_all": egl_call(outs["egl_all"])}
    times = {k: [] for k in calls}
    for it in range(1 + a.repeats):                        # the first walk warms every kernel up
        for name, fn in calls.items():
            ms, _ = _call_ms(fn)
            if it:
                times[name].append(ms)
    flops = {"forward": 2.0 * P * (D * a.h1 + a.h1 * a.h2)}
    flops["egl"] = flops["egl_all"] = 2.0 * P * (D * a.h1 + 2 * a.h1 * a.h2)
    res = {"shape": {"P": P, "D": D, "h1": a.h1, "h2": a.h2, "out_dim": 2, "pool_images": n, "gallery_images": g}, "repeats": a.repeats,
           "peak_f32_matrix_flops": PEAK_F32_MATRIX,
           "probabilities_equal_the_forwards_bits": bool(torch.equal(outs["egl_all"]["probs"], outs["forward"])),
           "egl_alone_equals_egl_of_all_bits": bool(torch.equal(outs["egl"]["egl"], outs["egl_all"]["egl"]))}
    for name, ms in times.items():
        med = float(np.median(ms))
        res[name] = {"ms_per_call": round(med, 4), "ms_per_call_min": round(float(np.min(ms)), 4), "flop": flops[name],
                     "flop_per_s": round(flops[name] / (med * 1e-3), -9), "share_of_f32_matrix_peak": round(flops[name] / (med * 1e-3) / PEAK_F32_MATRIX, 4)}
    res["egl_over_forward"] = round(res["egl"]["ms_per_call"] / res["forward"]["ms_per_call"], 3)
    res["egl_all_over_forward"] = round(res["egl_all"]["ms_per_call"] / res["forward"]["ms_per_call"], 3)
    res["egl_over_forward_by_operation_count"] = round(flops["egl"] / flops["forward"], 3)
    e = outs["egl"]["egl"]
    res["egl_values"] = {"min": float(e.min()), "median": float(e.median()), "max": float(e.max()), "zeros": int((e == 0).sum())}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
