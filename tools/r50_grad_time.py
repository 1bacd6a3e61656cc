"""Time of the VGGFace2 ResNet-50's input-gradient pass next to its forward, printed as one JSON line.

At --batch images (default 128) in --dtype (default bf16): the plain forward (alink_resnet50_embed), the cached forward
(alink_resnet50_embed_cached) and the backward (alink_resnet50_input_grad), each timed with HIP events over --reps calls
after warm-up, median of --rounds such windows; the backward as a multiple of the forward measured in the same run; and the
backward's stages (alink_resnet50_input_grad_profile: pooled map, the 16 units, max-pool, stem), median per stage.
An input-gradient pass has the forward's FLOP count, so a multiple far above 2 points at one stage.

    python tools/r50_grad_time.py [--batch 128] [--dtype bf16] [--reps 10] [--rounds 7]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STAGES = ["avg_pool"] + ["conv%d_%d" % (s + 2, u) for s in (3, 2, 1, 0) for u in range((3, 4, 6, 3)[s], 0, -1)] + ["max_pool", "stem"]


def _window_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    import a_link_amd  # noqa: F401
    from a_link_amd import _abi
    from a_link_amd.resnet50 import VGGResNet50
    from oracle import vgg_resnet50 as O
    n = args.batch
    net = VGGResNet50(dtype=args.dtype, max_batch=n, enable_grad=True)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, (n, 224, 224, 3)).astype(np.float32)).cuda()
    dfeat = torch.from_numpy(rng.standard_normal((n, 2048)).astype(np.float32)).cuda()
    out = torch.empty((n, 2048), dtype=torch.float32, device="cuda")
    dpix = torch.empty((n, 224, 224, 3), dtype=torch.float32, device="cuda")
    lib, st = net.lib, _abi.current_stream(net.device)
    ws, wsb = net.ws.get(n)
    gws, gwsb = net.ws.get(n, "grad")

    def fwd():
        _abi.check(lib.alink_resnet50_embed(net.h, _abi.ptr(x), n, 0, _abi.ptr(out), C.c_void_p(ws), wsb, st), "embed")

    def fwd_cached():
        _abi.check(lib.alink_resnet50_embed_cached(net.h, _abi.ptr(x), n, 0, _abi.ptr(out), C.c_void_p(gws), gwsb, st), "embed_cached")

    def bwd():
        _abi.check(lib.alink_resnet50_input_grad(net.h, _abi.ptr(dfeat), n, 0, _abi.ptr(dpix), C.c_void_p(gws), gwsb, st), "input_grad")

    for f in (fwd, fwd_cached, bwd):          # warm-up: code objects, every shape
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    t = {"forward": [], "forward_cached": [], "backward": []}
    for _ in range(args.rounds):              # the three interleaved, so that drift hits them alike
        t["forward"].append(_window_ms(fwd, args.reps))
        t["forward_cached"].append(_window_ms(fwd_cached, args.reps))
        t["backward"].append(_window_ms(bwd, args.reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    stages = []
    for _ in range(args.rounds):
        ms, k = (C.c_float * 32)(), C.c_int(32)
        _abi.check(lib.alink_resnet50_input_grad_profile(net.h, _abi.ptr(dfeat), n, 0, _abi.ptr(dpix), C.c_void_p(gws), gwsb, st, ms,
                                                         C.byref(k)), "input_grad_profile")
        stages.append([ms[i] for i in range(k.value)])
    stage_med = [statistics.median(c) for c in zip(*stages)]
    gflop = O.flops_per_image() * n / 1e9
    res = {"batch": n, "dtype": args.dtype, "timer": "HIP events", "measured": True, "reps": args.reps, "rounds": args.rounds,
           "forward_ms": round(med["forward"], 4), "forward_cached_ms": round(med["forward_cached"], 4),
           "backward_ms": round(med["backward"], 4),
           "spread_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
           "backward_over_forward": round(med["backward"] / med["forward"], 3),
           "forward_TFLOPs": round(gflop / med["forward"], 1), "backward_TFLOPs_at_forward_flops": round(gflop / med["backward"], 1),
           "stem_backward_ms": round(stage_med[-1], 4),
           "stem_backward_GFLOPs": round(2.0 * n * 224 * 224 * 12.25 * 64 * 3 / stage_med[-1] / 1e6, 1),
           "stages_ms": {name: round(v, 4) for name, v in zip(STAGES, stage_med)},
           "grad_workspace_MB": round(gwsb / 2.0 ** 20, 1), "forward_workspace_MB": round(wsb / 2.0 ** 20, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
