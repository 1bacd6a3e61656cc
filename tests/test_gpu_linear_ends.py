"""The two ends of conv3x3_linear_kernel: the prologue's bias / slope tables (loaded in one batch into registers, written to LDS
under run-time predicates) and the 16-bit epilogue's two forms (straight-line for a workgroup whose 224 pixels all exist,
predicated for a launch's ragged last group).

Every launch has the latency form off and asserts the kernel and form the entry reports: at these sizes the default setting
would run conv3x3_lat_kernel and the tests would test nothing.  Tolerances against the CPU reference are the project's
(tests/test_gpu_conv_forms.py: |err| <= rel |ref| + 2e-3, rel = 2^-8 bf16 / 2^-10 f16); everything else is bit equality."""
import pytest
import torch

from test_gpu_conv_forms import (Case, run16, check16, bits, restore, LINEAR_OF_W, SELF,
                                 PRELU, RESID, DACT, RESID_RELU, PRELU_RESID)

pytestmark = pytest.mark.gpu

EPILOGUES = [PRELU, RESID, PRELU_RESID, DACT, RESID_RELU]


def _head_of(big, n):
    """The first n images of `big` as a case of their own: same input, weights, tables, residual / dact."""
    N, H, W, Ci, Co, k, s, p = big.shape
    c = Case(0, big.dt, n, H, W, Ci, Co, k=k, s=s, p=p, reference=False, **big.flags)
    c.w, c.bias, c.alpha = big.w, big.bias, big.alpha
    c.x = big.x[:n].contiguous()
    c.resid = big.resid[:n].contiguous() if big.resid is not None else None
    c.dact = big.dact[:n].contiguous() if big.dact is not None else None
    return c


# (width, images in the ragged launch, images in the launch where the same pixels lie in full groups)
#   14: 196 pixels = one ragged group        | 8 x 196 = 1568 = 7 full groups
#   28: 784 = 3 full groups + 112 pixels     | 2 x 784 = 1568 = 7 full groups
#    7: 4 x 49 = 196 = one ragged group      | 32 x 49 = 1568 = 7 full groups
RAGGED_VS_FULL = [(14, 1, 8), (28, 1, 2), (7, 4, 32)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("W,n_small,n_big", RAGGED_VS_FULL)
def test_full_group_path_equals_ragged_path(gpu, dt, W, n_small, n_big):
    lib = gpu.load()
    assert (n_small * W * W) % 224 != 0 and (n_big * W * W) % 224 == 0
    try:
        lib.alink_debug_set_latency_form(0)
        for i, epi in enumerate(EPILOGUES):
            big = Case(3000 + 10 * W + i, dt, n_big, W, W, 128, 256, **epi)
            small = _head_of(big, n_small)
            for fine in (0, 1):
                full, _, _ = run16(gpu, big, route=1, fine=fine, expect=(LINEAR_OF_W[W], SELF))
                check16(full, big, "full groups fine=%d" % fine)
                ragged, _, _ = run16(gpu, small, route=1, fine=fine, expect=(LINEAR_OF_W[W], SELF))
                assert torch.isfinite(ragged.float()).all()
                assert torch.equal(bits(ragged), bits(full[:n_small])), (
                    "the ragged last group and a full group computed different bits for the same pixels", W, epi, fine)
    finally:
        restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_full_groups_at_56_wide(gpu, dt):
    """3136 pixels = 14 groups: a 56-wide square map is never ragged, so the straight-line form alone, against the reference
    (one form only at this width: `fine` is accepted and changes nothing)."""
    lib = gpu.load()
    try:
        lib.alink_debug_set_latency_form(0)
        for i, epi in enumerate(EPILOGUES):
            c = Case(3600 + i, dt, 1, 56, 56, 64, 128, **epi)
            outs = []
            for fine in (0, 1):
                out, _, _ = run16(gpu, c, route=1, fine=fine, expect=(LINEAR_OF_W[56], SELF))
                check16(out, c, "fine=%d" % fine)
                outs.append(out)
            assert torch.equal(bits(outs[0]), bits(outs[1]))
    finally:
        restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("Cout", [128, 384])
@pytest.mark.parametrize("border", [0, 1])
def test_table_slots(gpu, dt, Cout, border):
    """One bias row or nine (at nine the last load trip of the 128-channel form is half empty), slopes present or absent,
    one or three channel blocks (six in the 64-channel form: n0 != 0); Case's bias differs per class and channel.
    392 pixels: one full group and one ragged one, so both epilogue forms read the tables."""
    lib = gpu.load()
    try:
        lib.alink_debug_set_latency_form(0)
        for i, epi in enumerate([dict(alpha=1), dict(resid=1), dict(), dict(alpha=1, resid=1)]):
            c = Case(3700 + 4 * border + i, dt, 2, 14, 14, 64, Cout, border=border, **epi)
            assert (c.alpha is not None) == bool(epi.get("alpha")) and c.bias.shape == (9 if border else 1, Cout)
            outs = []
            for fine in (0, 1):
                for generic in (0, 1):                               # PReLU only / residual only: compile-time vs generic
                    lib.alink_debug_set_generic_epilogue(generic)
                    out, _, _ = run16(gpu, c, route=1, fine=fine, expect=(LINEAR_OF_W[14], SELF))
                    check16(out, c, "fine=%d generic=%d" % (fine, generic))
                    outs.append(out)
            for o in outs[1:]:
                assert torch.equal(bits(outs[0]), bits(o)), ("a form of the linear-tile kernel changed a bit", Cout, border, epi)
    finally:
        restore(lib)
