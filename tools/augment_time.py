"""Time of --augment's device work per fine-tune, printed as one JSON line.

For |q| queried pairs, helpers.augment_data makes 4 |q| images per side (original, rotation, shear, shift): one
alink_affine_warp launch per side, gathered out of a table of |q| source images.  Timed with HIP events (the launch
only, after warm-up), at 112 x 112 (ArcFace, ALINK_arc.py) and 224 x 224 (VGGFace2 ResNet-50, ALINK.py), next to the
time the loop spends embedding the 3 |q| transformed copies of one side in the exact mode (the originals reuse the
clean features).

    python tools/augment_time.py [--queries 250] [--reps 20]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--queries", type=int, default=250, help="|q|: queried pairs per fine-tune")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import a_link_amd  # noqa: F401
    from a_link_amd import _abi, augment, siamese
    n = args.queries
    out = {"queries": n, "images_per_side": 4 * n, "timer": "HIP events", "measured": True}
    for H, model in ((112, lambda: siamese.ArcFace((112, 112), "synthetic:r100:1")),
                     (224, lambda: siamese.RESNET50((224, 224)))):
        rng = np.random.default_rng(H)
        table = torch.from_numpy(rng.integers(0, 256, (n, H, H, 3)).astype(np.float32)).cuda()
        np.random.seed(0)
        plan = augment.draw(n, H, H, 1)
        # the kernel alone: the maps, sources and flags already on the device, as the warp of one side launches them
        d_mat = torch.from_numpy(np.ascontiguousarray(plan.maps[0])).cuda()
        d_src = torch.from_numpy(plan.src.astype(np.int32)).cuda()
        d_copy = torch.from_numpy(plan.copy[0].astype(np.uint8)).cuda()
        dst = torch.empty((len(plan.src), H, H, 3), dtype=torch.float32, device="cuda")
        lib = _abi.init(0)

        def launch():
            _abi.check(lib.alink_affine_warp(_abi.ptr(table), n, _abi.ptr(d_src), _abi.ptr(d_mat), _abi.ptr(d_copy), len(plan.src),
                                             H, H, 3, 1, _abi.ptr(dst), _abi.current_stream()), "alink_affine_warp")
        kernel_ms = _events_ms(launch, args.reps)
        # what the loop calls per side: draw's maps uploaded, the warp of the 3 |q| transformed rows
        new = ~plan.original
        warp_ms = _events_ms(lambda: augment.warp(table, plan.src[new], plan.maps[0][new], 1, plan.copy[0][new]), args.reps)
        copies = augment.warp(table, plan.src[new], plan.maps[0][new], 1, plan.copy[0][new])
        fm = model()
        embed_ms = _events_ms(lambda: fm.process(copies), max(1, args.reps // 10))
        nbytes = 2 * dst.numel() * 4
        out["%d" % H] = {"warp_kernel_ms": round(kernel_ms, 4), "warp_call_ms": round(warp_ms, 4),
                         "kernel_GBps_write_plus_read": round(nbytes / kernel_ms / 1e6, 1),
                         "embed_copies_ms": round(embed_ms, 3), "copies_embedded": int(new.sum())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
