"""GPU: csrc/unit1_c64.hip — the stem and the whole first residual unit (conv1 + PReLU, stride-2 conv2 + projection shortcut)
as one rolling-row launch, neither conv1's output nor the shortcut's operand leaving LDS, against the two launches it replaces
(alink_debug_set_fuse_unit1(0): the fused front kernel + the direct stride-2 kernel).  The same products are summed in the same
order and rounded at the same places, so the embeddings are equal bit for bit.  Small nets: stage 1 dominates and nothing
downstream masks a wrong bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = (1, 1, 1, 1)


def _embed(bb, x, lib, mode):
    lib.alink_debug_set_fuse_unit1(mode)
    try:
        return bb.embed_device(x).clone()
    finally:
        lib.alink_debug_set_fuse_unit1(1)


def _pixels(rng, n):
    return torch.from_numpy(rng.integers(0, 256, (n, 112, 112, 3), dtype=np.uint8)).cuda()


# the SURVEY weight draw (BatchNorm statistics as drawn) for bf16, the normalized draw for f16 (its range)
@pytest.mark.parametrize("units", ["r18", SMALL], ids=["r18", "u1111"])
@pytest.mark.parametrize("dtype,normalized", [("bf16", False), ("f16", True)])
def test_fused_unit1_is_bit_identical_to_two_launches(gpu, dtype, normalized, units):
    """1 and 3 images: fewer output rows than CUs, one-row ranges that start mid-image and on an image's first and last rows;
    37 and 70: ranges of about 8 and 15 output rows that cross image boundaries at odd offsets, 70 above the dispatch's
    threshold (mode 1); the others forced (mode 2).  One stream and two."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    u = W.ARCH_UNITS[units] if isinstance(units, str) else units
    params = W.synthetic_ir_params(u, seed=17, normalized=normalized)
    rng = np.random.default_rng(23)
    xs = {n: _pixels(rng, n) for n in (1, 3, 37, 70)}
    for streams in (1, 2):
        bb = IRBackbone(params, dtype=dtype, max_batch=128, streams=streams, lazy_range_check=True)
        for n, mode in ((1, 2), (3, 2), (37, 2), (70, 1)):
            plain = _embed(bb, xs[n], lib, 0)
            assert torch.isfinite(plain).all()
            fused = _embed(bb, xs[n], lib, mode)
            assert torch.equal(fused, plain), (streams, n, mode, (fused - plain).abs().max().item())


def test_fused_unit1_two_chunks_on_two_streams(gpu):
    """300 images at max_batch 292: two chunks, on two streams."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    params = W.synthetic_ir_params(W.ARCH_UNITS["r18"], seed=17, normalized=False)
    bb = IRBackbone(params, dtype="bf16", max_batch=292, streams=2, lazy_range_check=True)
    x = _pixels(np.random.default_rng(29), 300)
    plain = _embed(bb, x, lib, 0)
    assert torch.isfinite(plain).all()
    for mode in (1, 2):
        fused = _embed(bb, x, lib, mode)
        assert torch.equal(fused, plain), (mode, (fused - plain).abs().max().item())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_unit1_every_pixel_layout_and_slopes_above_one(gpu, dtype):
    """NHWC u8, NHWC f32 and NCHW f32 pixels; then per-channel PReLU slopes on both sides of 1 in the stem and in conv1, so
    that the compare / select form of the PReLU runs instead of the max form."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    params = W.synthetic_ir_params(SMALL, seed=5, normalized=True)
    u8 = _pixels(np.random.default_rng(11), 5)
    layouts = (u8, u8.float(), u8.float().permute(0, 3, 1, 2).contiguous())
    bb = IRBackbone(params, dtype=dtype, max_batch=8)
    for x in layouts:
        plain, fused = _embed(bb, x, lib, 0), _embed(bb, x, lib, 2)
        assert torch.isfinite(plain).all()
        assert torch.equal(fused, plain), (x.dtype, tuple(x.shape), (fused - plain).abs().max().item())
    steep = dict(params)
    rng = np.random.default_rng(3)
    for name in ("relu0_gamma", "stage1_unit1_relu1_gamma"):
        steep[name] = rng.uniform(0.1, 1.5, np.asarray(params[name]).shape).astype(np.float32)
        assert (steep[name] > 1).any() and (steep[name] < 1).any()
    bb = IRBackbone(steep, dtype=dtype, max_batch=8)
    for x in layouts[:2]:
        plain, fused = _embed(bb, x, lib, 0), _embed(bb, x, lib, 2)
        assert torch.isfinite(plain).all()
        assert torch.equal(fused, plain), (x.dtype, (fused - plain).abs().max().item())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_unit1_profile_keeps_one_entry_per_layer(gpu, dtype):
    """bb.profile() keeps one convolution entry per layer (bench.py's roofline maps entries to layer shapes): the launch
    appears as s1u1 conv1 (+ stem FLOPs) and s1u1 conv2 (+ shortcut), each with its own FLOPs and half of the launch's time."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    from oracle import ir_resnet
    units = W.ARCH_UNITS["r18"]
    lib = gpu.load()
    bb = IRBackbone(W.synthetic_ir_params(units, seed=3, normalized=True), dtype=dtype, max_batch=70)
    x = _pixels(np.random.default_rng(5), 70)
    fused = bb.profile(x)
    lib.alink_debug_set_fuse_unit1(0)
    try:
        plain = bb.profile(x)
    finally:
        lib.alink_debug_set_fuse_unit1(1)
    assert [k for k, _, _ in fused] == [k for k, _, _ in plain]
    assert [k for k, _, _ in fused].count(1) == 2 * sum(units)
    assert [f for _, _, f in fused] == [f for _, _, f in plain]
    total = sum(f for _, _, f in fused)
    assert abs(total / 70 - ir_resnet.flops_per_image(units, size=112)) < 1e-6 * total
    convs = [ms for k, ms, _ in fused if k == 1]
    assert convs[0] > 0 and convs[0] == convs[1], convs[:2]
    assert all(ms >= 0 for _, ms, _ in fused)
    # the two launches have times of their own
    convs = [ms for k, ms, _ in plain if k == 1]
    assert convs[0] > 0 and convs[1] > 0 and convs[0] != convs[1], convs[:2]


def test_fused_unit1_gives_way_to_the_front_and_stride2_switches(gpu):
    """alink_debug_set_fuse_stem(0) and alink_debug_set_s2direct(0) keep selecting what they selected before the fused launch
    existed, so each turns it off: a stem launch of its own (profile kind 0) in the first case, two s1u1 launches with
    times of their own in the second — and the same bits either way."""
    from a_link_amd import weights as W
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    params = W.synthetic_ir_params(SMALL, seed=7, normalized=True)
    bb = IRBackbone(params, dtype="bf16", max_batch=70)
    x = _pixels(np.random.default_rng(13), 70)
    plain = _embed(bb, x, lib, 0)
    lib.alink_debug_set_fuse_unit1(2)
    try:
        assert bb.profile(x)[0][0] == 1
        lib.alink_debug_set_fuse_stem(0)
        try:
            assert bb.profile(x)[0][0] == 0
            a = bb.embed_device(x).clone()
        finally:
            lib.alink_debug_set_fuse_stem(1)
        lib.alink_debug_set_s2direct(0)
        try:
            convs = [ms for k, ms, _ in bb.profile(x) if k == 1]
            assert convs[0] != convs[1], convs[:2]
            b = bb.embed_device(x).clone()
        finally:
            lib.alink_debug_set_s2direct(1)
    finally:
        lib.alink_debug_set_fuse_unit1(1)
    assert torch.equal(a, plain) and torch.equal(b, plain)
