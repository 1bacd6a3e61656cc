"""GPU: csrc/unit_c64.hip — a plain stage-1 residual unit (56 x 56 x 64: conv1 + PReLU, conv2 + residual) as one rolling-row
launch with conv1's output kept in LDS, against the two linear-tile launches it replaces (alink_debug_set_fuse_unit(0)).
The same products are summed in the same order and rounded at the same places, so the embeddings are equal bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _embed(bb, x, lib, mode):
    lib.alink_debug_set_fuse_unit(mode)
    try:
        return bb.embed_device(x).clone()
    finally:
        lib.alink_debug_set_fuse_unit(1)


# the SURVEY weight draw (BatchNorm statistics as drawn) leaves the f16 range in deep IR-100 stages: f16 on normalized draws
@pytest.mark.parametrize("dtype,arch,normalized", [("bf16", "r100", False), ("bf16", "r50", True),
                                                   ("f16", "r100", True), ("f16", "r50", True)])
def test_fused_unit_is_bit_identical_to_two_launches(gpu, dtype, arch, normalized):
    """Batches whose workgroup ranges start mid-image and at image edges (3: fewer pass pairs than CUs, one pair per range;
    83 and 300: ranges that cross image boundaries; 1168: the bench's whole step in one call, sharded), the fused form
    forced at every batch size (mode 2) and at its default threshold (mode 1), on one stream and on four."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    params = W.synthetic_ir_params(W.ARCH_UNITS[arch], seed=17, normalized=normalized)
    rng = np.random.default_rng(23)
    for streams in (1, 4):
        bb = IRBackbone(params, dtype=dtype, max_batch=292, streams=streams, lazy_range_check=True)
        for n in (3, 83, 300, 1168):
            x = torch.from_numpy(rng.integers(0, 256, (n, 112, 112, 3), dtype=np.uint8)).cuda()
            plain = _embed(bb, x, lib, 0)
            assert torch.isfinite(plain).all()
            for mode in (2, 1):
                fused = _embed(bb, x, lib, mode)
                assert torch.equal(fused, plain), (streams, n, mode, (fused - plain).abs().max().item())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_unit_profile_keeps_one_entry_per_layer(gpu, dtype):
    """bb.profile() keeps one convolution entry per layer of the chain (bench.py's roofline maps entries to layer shapes):
    a fused unit's launch appears as its conv1 and conv2, each with its own FLOPs and half of the launch's time."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    from oracle import ir_resnet
    units = W.R50_UNITS
    lib = gpu.load()
    bb = IRBackbone(W.synthetic_ir_params(units, seed=3, normalized=True), dtype=dtype, max_batch=128)
    x = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (128, 112, 112, 3), dtype=np.uint8)).cuda()
    fused = bb.profile(x)
    lib.alink_debug_set_fuse_unit(0)
    try:
        plain = bb.profile(x)
    finally:
        lib.alink_debug_set_fuse_unit(1)
    assert [k for k, _, _ in fused] == [k for k, _, _ in plain]
    assert [k for k, _, _ in fused].count(1) == 2 * sum(units)
    assert [f for _, _, f in fused] == [f for _, _, f in plain]
    total = sum(f for _, _, f in fused)
    assert abs(total / 128 - ir_resnet.flops_per_image(units, size=112)) < 1e-6 * total
    # conv entries in chain order: s1u1 conv1 (+ stem), s1u1 conv2 (+ shortcut), then s1u2 conv1, s1u2 conv2, ...
    convs = [ms for k, ms, _ in fused if k == 1]
    for u in range(1, units[0]):
        a, b = convs[2 * u], convs[2 * u + 1]
        assert a > 0 and a == b, (u, a, b)
    assert all(ms >= 0 for _, ms, _ in fused)
