"""The input-span refill of conv3x3_linear_kernel's main loop: requested inside a 64-channel chunk's last K-step, under the MFMAs
of its second k-half (the default), against the form that refills after the step and waits with nothing else in flight
(alink_debug_set_early_refill(0)).  Both run the same MFMAs on the same operands in the same order, so every comparison between
them is on raw bits; against the CPU reference the tolerance is the project's (tests/test_gpu_conv_forms.py).

Every launch has the latency form off and asserts the kernel and form the entry reports: at these sizes the default setting
would run conv3x3_lat_kernel, which has no refill."""
import numpy as np
import pytest
import torch

from test_gpu_conv_forms import (Case, run16, check16, runx2, checkx2, bits, restore, LINEAR_OF_W, SELF,
                                 PRELU, RESID, DACT, RESID_RELU, PRELU_RESID)

pytestmark = pytest.mark.gpu

EPILOGUES = [PRELU, RESID, PRELU_RESID, DACT, RESID_RELU]

# (width, images, Cin, Cout): the smallest launches that still contain each case
SHAPES = [
    (14, 1, 128, 128),     # one ragged group, 1 refill
    (14, 8, 256, 256),     # 7 full groups crossing image boundaries, 3 refills
    (28, 2, 128, 128),     # full groups, 1 refill
    (7, 4, 256, 256),      # one ragged group, 3 refills
    (7, 32, 512, 512),     # full groups, 7 refills
    (56, 1, 128, 128),     # 1 refill at the widest halo
    (14, 1, 64, 128),      # one chunk, no refill: the switch must change nothing (128 outputs: at 14 wide the linear-tile
                           # kernel serves Cout % 128 == 0 only, a 64 -> 64 layer there runs the implicit GEMM)
]


def _restore(lib):
    lib.alink_debug_set_early_refill(1)
    restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("W,N,Ci,Co", SHAPES)
def test_early_refill_equals_late_refill(gpu, dt, W, N, Ci, Co):
    lib = gpu.load()
    try:
        lib.alink_debug_set_latency_form(0)
        for i, epi in enumerate(EPILOGUES):
            c = Case(4000 + 100 * W + Ci + i, dt, N, W, W, Ci, Co, **epi)
            for fine in (0, 1):
                outs = []
                for early in (1, 0):
                    lib.alink_debug_set_early_refill(early)
                    out, _, _ = run16(gpu, c, route=1, fine=fine, expect=(LINEAR_OF_W[W], SELF))
                    check16(out, c, "fine=%d early=%d" % (fine, early))
                    outs.append(out)
                assert torch.equal(bits(outs[0]), bits(outs[1])), ("the early refill changed a bit", dt, (W, N, Ci, Co), epi, fine)
    finally:
        _restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_k_split_slabs(gpu, dt):
    """An IRBackbone with small_batch_split: each slab of a split launch walks ncc / splitk chunks from its own first one, with
    the refills between them.  1 and 3 images of a (1, 1, 1, 1) net, switch on against switch off."""
    from a_link_amd import weights as Wt
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    params = Wt.synthetic_ir_params((1, 1, 1, 1), seed=7, normalized=True)
    x = np.random.default_rng(5).integers(0, 256, (3, 112, 112, 3), dtype=np.uint8)
    bb = IRBackbone(params, dtype=dt, max_batch=4, small_batch_split=True)
    try:
        lib.alink_debug_set_latency_form(0)
        for n in (1, 3):
            lib.alink_debug_set_early_refill(1)
            on = bb.embed(x[:n])
            lib.alink_debug_set_early_refill(0)
            off = bb.embed(x[:n])
            assert np.isfinite(on).all() and np.allclose(np.linalg.norm(on, axis=1), 1.0, atol=1e-5)
            assert np.array_equal(on.view(np.int32), off.view(np.int32)), (dt, n, np.abs(on - off).max())
    finally:
        _restore(lib)


@pytest.mark.parametrize("W,N,Ci,Co", [s for s in SHAPES if s[0] in (14, 7)])
def test_split_precision(gpu, W, N, Ci, Co):
    """f16x2 refills twice per chunk (after the hi half's second walk, and at the chunk end); the one-product screening form
    once.  Both are on the early form: switch on equals switch off, in the 64- and the 128-channel form."""
    lib = gpu.load()
    try:
        lib.alink_debug_set_latency_form(0)
        for i, epi in enumerate([PRELU, RESID, PRELU_RESID, RESID_RELU]):          # (split precision has no backward epilogue)
            c = Case(4500 + 100 * W + Ci + i, "x2", N, W, W, Ci, Co, **epi)
            for nprod in (3, 1):
                for fine in (0, 1):
                    outs = []
                    for early in (1, 0):
                        lib.alink_debug_set_early_refill(early)
                        out = runx2(gpu, c, fine=fine, nprod=nprod, expect=(LINEAR_OF_W[W], SELF))
                        checkx2(out, c, nprod, "fine=%d early=%d" % (fine, early))
                        outs.append(out)
                    assert torch.equal(bits(outs[0]), bits(outs[1])), ("the early refill changed a bit", (W, N, Ci, Co), epi, nprod, fine)
    finally:
        _restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("fine_max", [384, 100000])
def test_concurrent_launches_equal_serial(gpu, dt, fine_max):
    """A refill that overtook another wave's fragment reads would show only with launches overlapping on several streams (as
    the missing read wait of round 3 did: conv_device.h wait_then_barrier).  600 images of a (1, 2, 2, 1) net at 112 x 112 as
    150-image launches on four streams, eight times, against the one-stream result: every bit equal — with the 64-channel
    form forced everywhere (fine_max = 100000) and at the dispatch's own choice."""
    from a_link_amd import weights as Wt
    from a_link_amd.backbone import IRBackbone
    lib = gpu.load()
    lib.alink_debug_set_fine_max(fine_max)
    try:
        p = Wt.synthetic_ir_params((1, 2, 2, 1), seed=1, normalized=True)
        x = torch.randint(0, 256, (600, 112, 112, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
        ref = IRBackbone(p, dtype=dt, max_batch=150, streams=1).embed_device(x).clone()
        assert torch.isfinite(ref).all()
        bb = IRBackbone(p, dtype=dt, max_batch=150, streams=4)
        for rep in range(8):
            got = bb.embed_device(x)
            torch.cuda.synchronize()
            bad = torch.nonzero((got != ref).any(1)).flatten().tolist()
            assert not bad, (dt, fine_max, rep, len(bad), bad[:16])
    finally:
        lib.alink_debug_set_fine_max(384)
