"""Per-layer parity of every convolution kernel, launch form and epilogue through alink_conv_nhwc_ex / alink_conv_nhwc_x2_ex,
against a CPU convolution of the same (rounded) operands.  Every case asserts the kernel and the form the entry REPORTS, so a
case cannot silently run something other than what it was written for.

Tolerances are the project's own (tests/test_gpu_conv.py): 16-bit |err| <= rel |ref| + 2e-3 with rel = 2^-8 (bf16) / 2^-10 (f16),
also for the K-split results (they differ from the fused ones in f32 summation order only); split precision err / sum|products|
< 4e-6 with three products and < 1e-3 with one (each operand one f16 rounding, 2^-11: 2^-10 (1 + 2^-11) + 4e-6 = 9.8e-4).
Where the project promises bit identity (latency form vs tile kernel, 64- vs 128-channel form, compile-time vs generic
epilogue) the raw bits are compared."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# ConvKernel (a-link_amd/csrc/conv_kernel.h)
IGEMM, D1, D2, D3, D4, D5, D6, S1, S3 = 0, 1, 2, 3, 4, 5, 6, 7, 8
LIN14, LIN28, LIN56, LIN7, LIN112, ROLL112, ROLL112S2 = 11, 12, 13, 14, 15, 21, 25
LINEAR_OF_W = {7: LIN7, 14: LIN14, 28: LIN28, 56: LIN56, 112: LIN112}
# forms
SELF, LAT3X3, LATGEMM = 0, 1, 2

# epilogues: (border classes, PReLU, residual, dact, post_relu)
PRELU = dict(border=1, alpha=1)
RESID = dict(resid=1)
DACT = dict(border=1, alpha=1, dact=1)
RESID_RELU = dict(resid=1, post_relu=1)
PRELU_RESID = dict(border=1, alpha=1, resid=1)
FOUR = [PRELU, RESID, DACT, RESID_RELU]


def _tdt(dt):
    return torch.bfloat16 if dt == "bf16" else torch.float16


def _out_hw(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


class Case:
    """Operands of one convolution (rounded to the 16-bit type, or float32 for split precision) and its CPU reference."""

    def __init__(self, seed, dt, N, H, W, Ci, Co, k=3, s=1, p=1, border=0, alpha=0, resid=0, dact=0, post_relu=0, Cin2=0, compact=0,
                 nan_at=None, reference=True):
        g = torch.Generator().manual_seed(seed)
        self.dt, self.shape = dt, (N, H, W, Ci, Co, k, s, p)
        self.flags = dict(border=border, alpha=alpha, resid=resid, dact=dact, post_relu=post_relu, Cin2=Cin2, compact=compact)
        t = torch.float32 if dt == "x2" else _tdt(dt)
        hi = torch.float64 if dt == "x2" else torch.float32         # the reference's precision
        Ho, Wo = _out_hw(H, W, k, s, p)
        self.Ho, self.Wo = Ho, Wo
        self.x = torch.randn(N, H, W, Ci, generator=g).to(t)
        self.w = (torch.randn(Co, k, k, Ci, generator=g) / np.sqrt(k * k * Ci)).to(t)
        self.bias = torch.randn(9 if border else 1, Co, generator=g)
        self.alpha = torch.rand(Co, generator=g) * 0.5 if alpha else None
        self.resid = torch.randn(N, Ho, Wo, Co, generator=g).to(t) if resid else None
        self.dact = None
        if dact:
            d = torch.randn(N, Ho, Wo, Co, generator=g)
            flat = d.view(-1)
            flat[::7] = 0.0                                          # exact zeros and -0.0: both take the slope
            flat[3::11] = -0.0
            self.dact = d.to(t)
        if nan_at is not None:
            self.resid.view(-1)[nan_at] = float("nan")
        self.in2 = self.w2 = None
        if Cin2:
            self.in2 = torch.randn(*((N, Ho, Wo) if compact else (N, H, W)), Cin2, generator=g).to(t)
            self.w2 = (torch.randn(Co, Cin2, generator=g) / np.sqrt(Cin2)).to(t)
        self.ref, self.mag = (self._reference(hi) if reference else None), None     # (a request the entry must refuse has none)
        if dt == "x2":                                               # sum |products| per output (no bias, no residual: the stricter scale)
            self.mag = F.conv2d(self.x.double().abs().permute(0, 3, 1, 2), self.w.double().abs().permute(0, 3, 1, 2),
                                stride=s, padding=p).permute(0, 2, 3, 1)

    def _reference(self, hi):
        N, H, W, Ci, Co, k, s, p = self.shape
        y = F.conv2d(self.x.to(hi).permute(0, 3, 1, 2), self.w.to(hi).permute(0, 3, 1, 2), stride=s, padding=p).permute(0, 2, 3, 1)
        bias = self.bias.to(hi)
        if self.flags["border"]:
            rc = torch.ones(self.Ho, dtype=torch.long); rc[0] = 0; rc[-1] = 2
            cc = torch.ones(self.Wo, dtype=torch.long); cc[0] = 0; cc[-1] = 2
            y = y + bias[rc[:, None] * 3 + cc[None, :]]
        else:
            y = y + bias[0]
        if self.in2 is not None:
            sc = F.conv2d(self.in2.to(hi).permute(0, 3, 1, 2), self.w2.to(hi)[:, :, None, None],
                          stride=1 if self.flags["compact"] else s).permute(0, 2, 3, 1)
            y = y + sc
        if self.dact is not None:
            return y * torch.where(self.dact.to(hi) > 0, torch.ones((), dtype=hi), self.alpha.to(hi))
        if self.alpha is not None:
            y = torch.where(y > 0, y, y * self.alpha.to(hi))
        if self.resid is not None:
            y = y + self.resid.to(hi)
        if self.flags["post_relu"]:
            y = torch.where(y < 0, torch.zeros((), dtype=hi), y)     # keeps a NaN, as the kernels do
        return y

    def cuda(self):
        if not hasattr(self, "_dev"):
            self._dev = {n: (getattr(self, n).cuda() if getattr(self, n) is not None else None)
                         for n in ("x", "w", "bias", "alpha", "resid", "dact", "in2", "w2")}
        return self._dev


def run16(gpu, c, route=0, fine=-1, splitk=1, expect=None, rc_only=False):
    """one launch through alink_conv_nhwc_ex into a NaN-filled output; returns (out, kernel, form)"""
    lib = gpu.load()
    N, H, W, Ci, Co, k, s, p = c.shape
    d = c.cuda()
    out = torch.full((N, c.Ho, c.Wo, Co), float("nan"), dtype=_tdt(c.dt), device="cuda")
    kern, form = C.c_int(-7), C.c_int(-7)
    rc = lib.alink_conv_nhwc_ex(gpu.DT_BF16 if c.dt == "bf16" else gpu.DT_F16, gpu.ptr(d["x"]), gpu.ptr(d["w"]), gpu.ptr(d["bias"]),
                                gpu.ptr(d["alpha"]), gpu.ptr(d["resid"]), gpu.ptr(out), N, H, W, Ci, Co, k, s, p, c.flags["border"], fine,
                                route, gpu.ptr(d["dact"]), c.flags["post_relu"], gpu.ptr(d["in2"]), gpu.ptr(d["w2"]), c.flags["Cin2"],
                                c.flags["compact"], splitk, C.byref(kern), C.byref(form), None)
    if rc_only:
        return rc, out
    gpu.check(rc, "alink_conv_nhwc_ex %s" % (c.shape,))
    if expect is not None:
        assert (kern.value, form.value) == expect, "case %s %s: ran kernel %d form %d, written for %s" % (
            c.shape, c.flags, kern.value, form.value, expect)
    return out, kern.value, form.value


def check16(out, c, what=""):
    got = out.float().cpu()
    assert torch.isfinite(got).all(), (c.shape, c.flags, what)
    rel = 2.0 ** -8 if c.dt == "bf16" else 2.0 ** -10
    err = (got - c.ref).abs()
    tol = rel * c.ref.abs() + 2e-3
    print("%s %s %s %s: max excess %.4g" % (c.dt, c.shape, c.flags, what, float((err - tol).max())))
    assert (err <= tol).all(), "case %s %s %s dt=%s: excess %.4g" % (c.shape, c.flags, what, c.dt, float((err - tol).max()))


def bits(t):
    return t.view(torch.int16) if t.dtype != torch.float32 else t.view(torch.int32)


def restore(lib):
    lib.alink_debug_set_linear(31)
    lib.alink_debug_set_pair(1)
    lib.alink_debug_set_dma(1)
    lib.alink_debug_set_latency_form(1600)
    lib.alink_debug_set_latency_tiles(-1)
    lib.alink_debug_set_generic_epilogue(0)


# ---- row-aligned tile kernels (D1..D6) and pair kernels (S1, S3) of conv3x3_direct.hip --------------------------------------
# Reached through direct_variant_tiles with the linear-tile kernel off; D1..D3 ONLY with the pair kernels off as well (the
# pair kernels take every Cout % 128 == 0 first).  Widths: both ends of every admitted range (12-14, 17-30, 49-62, 112) —
# a 16-column block with a single valid column (17, 49), the row pitch exactly W + 2 (14, 30, 62); row counts that are no
# multiple of the tile's rows, H = 1; two images; Cin of 64 (single X buffer), 128 (double) and 192.
TILE_SHAPES = {
    # kernel: (pair switch, four shapes (N, H, W, Cin, Cout))
    D1: (0, [(2, 13, 14, 64, 256), (2, 15, 12, 128, 256), (2, 1, 13, 192, 256), (2, 14, 14, 128, 512)]),
    D2: (0, [(2, 9, 17, 64, 256), (2, 8, 30, 128, 256), (2, 1, 28, 64, 256), (2, 15, 28, 128, 256)]),
    D3: (0, [(2, 9, 17, 128, 128), (2, 10, 30, 64, 128), (1, 30, 28, 64, 384), (2, 1, 17, 192, 128)]),
    D4: (0, [(2, 5, 49, 64, 128), (2, 6, 62, 128, 128), (2, 9, 56, 64, 256), (2, 1, 62, 192, 128)]),
    D5: (0, [(2, 9, 49, 64, 64), (2, 8, 62, 64, 64), (2, 13, 56, 64, 192), (2, 1, 56, 64, 64)]),        # Cin = 64 only: 128 does not fit
    D6: (0, [(2, 9, 112, 64, 64), (1, 1, 112, 64, 64), (2, 5, 112, 64, 128), (1, 6, 112, 64, 64)]),     # the same
    S1: (1, [(2, 13, 14, 64, 128), (2, 15, 12, 128, 256), (2, 1, 13, 192, 128), (2, 14, 14, 128, 128)]),
    S3: (1, [(2, 9, 17, 64, 128), (2, 8, 30, 128, 256), (2, 15, 28, 128, 128), (2, 1, 30, 192, 128)]),
}


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("kernel", sorted(TILE_SHAPES))
def test_tile_and_pair_kernels(gpu, dt, kernel):
    lib = gpu.load()
    pair, shapes = TILE_SHAPES[kernel]
    try:
        lib.alink_debug_set_linear(0)
        lib.alink_debug_set_pair(pair)
        for i, shp in enumerate(shapes):
            epi = FOUR[(i + kernel) % 4]                             # every kernel gets all four epilogues
            if shp[1] == 1:
                epi = dict(epi, border=0)                            # one row is top AND bottom border: none of the nine classes
            c = Case(1000 + 10 * kernel + i, dt, *shp, **epi)
            out, _, _ = run16(gpu, c, route=1, expect=(kernel, SELF))
            check16(out, c)
    finally:
        restore(lib)


def test_wide_cin_of_the_56_wide_64_channel_layer_falls_to_the_gemm(gpu):
    """TileW56C64 / TileW112C64 double-buffer X only while it fits 160 KB: Cin = 128 does not, and the chooser must hand the
    layer to the implicit GEMM instead of launching a tile kernel beyond its LDS."""
    lib = gpu.load()
    try:
        lib.alink_debug_set_linear(0)
        for shp in [(1, 9, 56, 128, 64), (1, 5, 112, 128, 64)]:
            c = Case(77, "bf16", *shp, **PRELU)
            out, _, _ = run16(gpu, c, route=1, expect=(IGEMM, SELF))
            check16(out, c)
    finally:
        restore(lib)


# ---- the linear-tile kernel proper (latency form off) -----------------------------------------------------------------------
LINEAR_SHAPES = [(9, 7, 7, 128, 128), (11, 14, 14, 128, 256), (3, 28, 28, 64, 128), (1, 56, 56, 64, 64)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("shp", LINEAR_SHAPES)
def test_linear_kernel_proper(gpu, dt, shp):
    """Every epilogue on launches the linear-tile kernel really serves; the 64- and 128-channel forms bit-equal; the
    compile-time epilogues (PReLU only, residual only) bit-equal to the generic one."""
    lib = gpu.load()
    W = shp[2]
    fines = (0, 1) if W != 56 else (0,)
    try:
        lib.alink_debug_set_latency_form(0)
        for i, epi in enumerate([PRELU_RESID, DACT, RESID_RELU, PRELU, RESID]):
            c = Case(2000 + i, dt, *shp, **epi)
            outs = []
            for fine in fines:
                for generic in ((0, 1) if epi in (PRELU, RESID) else (0,)):
                    lib.alink_debug_set_generic_epilogue(generic)
                    out, _, _ = run16(gpu, c, route=1, fine=fine, expect=(LINEAR_OF_W[W], SELF))
                    check16(out, c, "fine=%d generic=%d" % (fine, generic))
                    outs.append(out)
            for o in outs[1:]:
                assert torch.equal(bits(outs[0]), bits(o)), ("a form of the linear-tile kernel changed a bit", shp, epi)
    finally:
        restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_linear_kernel_k_split(gpu, dt):
    """K split per 64-channel chunk into f32 slabs + conv_split_finish, every epilogue of the finish kernel."""
    lib = gpu.load()
    try:
        lib.alink_debug_set_latency_form(0)
        for i, (shp, S, epi) in enumerate([((2, 7, 7, 256, 128), 2, PRELU_RESID), ((2, 7, 7, 256, 128), 4, DACT),
                                           ((9, 7, 7, 128, 128), 2, RESID_RELU), ((2, 14, 14, 256, 128), 4, PRELU),
                                           ((3, 14, 14, 128, 256), 2, DACT), ((1, 28, 28, 128, 128), 2, RESID),
                                           ((1, 56, 56, 128, 64), 2, PRELU_RESID)]):
            c = Case(2100 + i, dt, *shp, **epi)
            for fine in ((0, 1) if shp[2] != 56 else (0,)):
                out, _, _ = run16(gpu, c, route=1, fine=fine, splitk=S, expect=(LINEAR_OF_W[shp[2]], SELF))
                check16(out, c, "splitk=%d fine=%d" % (S, fine))
    finally:
        restore(lib)


# ---- the latency form of the 3x3 layers, per layer ----------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_latency_form_3x3(gpu, dt):
    """conv3x3_lat_kernel in each of its three block shapes: against the reference, and bit-equal to the linear-tile kernel."""
    lib = gpu.load()
    try:
        for i, (shp, epi) in enumerate([((1, 7, 7, 128, 128), PRELU), ((3, 7, 7, 128, 128), RESID_RELU),      # 147 pixels: no multiple of 16
                                        ((1, 14, 14, 128, 256), RESID), ((3, 14, 14, 256, 128), PRELU_RESID),
                                        ((1, 28, 28, 128, 128), RESID_RELU)]):
            c = Case(2200 + i, dt, *shp, **epi)
            kern = LINEAR_OF_W[shp[2]]
            lib.alink_debug_set_latency_form(0)
            base, _, _ = run16(gpu, c, route=1, fine=0, expect=(kern, SELF))
            check16(base, c, "linear")
            lib.alink_debug_set_latency_form(1600)
            for tiles in (0, 1, 2):
                lib.alink_debug_set_latency_tiles(tiles)
                out, _, _ = run16(gpu, c, route=1, expect=(kern, LAT3X3))
                check16(out, c, "latency tiles=%d" % tiles)
                assert torch.equal(bits(out), bits(base)), ("latency form differs from the linear-tile kernel", shp, tiles)
    finally:
        restore(lib)


# ---- implicit GEMM proper and its latency form --------------------------------------------------------------------------------
GEMM_CASES = [
    # (N, H, W, Cin, Cout, ksz, stride, pad), epilogue
    ((2, 14, 14, 64, 64, 3, 2, 1), RESID),
    ((1, 9, 9, 128, 64, 3, 2, 1), dict(alpha=1)),
    ((3, 14, 14, 256, 128, 3, 2, 1), RESID_RELU),
    ((1, 8, 8, 512, 128, 3, 2, 1), dict(alpha=1, resid=1)),
    ((3, 8, 8, 64, 128, 1, 2, 0), dict()),
    ((2, 14, 14, 128, 256, 1, 2, 0), RESID_RELU),
    ((2, 14, 14, 256, 128, 1, 1, 0), dict(alpha=1)),           # the backward shortcut's shape
    ((1, 8, 8, 512, 64, 1, 1, 0), RESID),
]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_and_its_latency_form(gpu, dt):
    lib = gpu.load()
    try:
        for i, (shp, epi) in enumerate(GEMM_CASES):
            c = Case(2300 + i, dt, *shp[:5], k=shp[5], s=shp[6], p=shp[7], **epi)
            lib.alink_debug_set_latency_form(0)
            outs = []
            for dma in (1, 0):
                lib.alink_debug_set_dma(dma)
                out, _, _ = run16(gpu, c, expect=(IGEMM, SELF))
                check16(out, c, "dma=%d" % dma)
                outs.append(out)
            lib.alink_debug_set_dma(1)
            lib.alink_debug_set_latency_form(1600)
            out, _, _ = run16(gpu, c, expect=(IGEMM, LATGEMM))
            check16(out, c, "latency")
            assert torch.equal(bits(out), bits(outs[0])), ("conv_gemm_lat_kernel differs from conv_igemm", shp)
    finally:
        restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_gemm_default_setting_backward_epilogue_and_k_split(gpu, dt):
    lib = gpu.load()
    try:
        # more than 784 output pixels: the library's default setting reaches conv_igemm itself
        # (980 pixels of a 1x1 layer), or more than 512 waves of 16 x 16 blocks (392 pixels x 512 channels of a stride-2 3x3 layer)
        for shp, epi in [((5, 14, 14, 64, 128, 1, 1, 0), RESID_RELU), ((2, 28, 28, 64, 512, 3, 2, 1), dict(alpha=1))]:
            c = Case(2400, dt, *shp[:5], k=shp[5], s=shp[6], p=shp[7], **epi)
            out, _, _ = run16(gpu, c, expect=(IGEMM, SELF))
            check16(out, c, "default")
        # dact (the latency form has none: conv_igemm serves it whatever the setting); 3x3 stride 1 at a width no tile kernel admits
        for shp, epi in [((2, 14, 14, 128, 64, 1, 1, 0), dict(alpha=1, dact=1)), ((2, 9, 16, 64, 128, 3, 1, 1), DACT),
                         ((1, 11, 15, 128, 64, 3, 1, 1), DACT)]:
            c = Case(2410, dt, *shp[:5], k=shp[5], s=shp[6], p=shp[7], **epi)
            out, _, _ = run16(gpu, c, route=1, expect=(IGEMM, SELF))
            check16(out, c, "dact")
        # K split per K-step, whole divisors of the K-steps
        for shp, S, epi in [((2, 14, 14, 128, 128, 3, 2, 1), 2, RESID_RELU), ((2, 14, 14, 128, 128, 3, 2, 1), 3, dict(alpha=1)),
                            ((2, 8, 8, 192, 128, 1, 1, 0), 3, dict(alpha=1, dact=1)), ((3, 8, 8, 256, 64, 1, 2, 0), 2, RESID),
                            ((2, 9, 16, 64, 128, 3, 1, 1), 3, PRELU_RESID)]:
            c = Case(2420 + S, dt, *shp[:5], k=shp[5], s=shp[6], p=shp[7], **epi)
            out, _, _ = run16(gpu, c, splitk=S, expect=(IGEMM, SELF))
            check16(out, c, "splitk=%d" % S)
    finally:
        restore(lib)


# ---- the fused 1x1 projection shortcut ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_fused_shortcut_gemm(gpu, dt):
    lib = gpu.load()
    try:
        i = 0
        for (Ci, Ci2) in ((128, 64), (256, 128)):
            for (N, HW) in ((3, 14), (2, 28)):
                for compact in (0, 1):
                    i += 1
                    c = Case(2500 + i, dt, N, HW, HW, Ci, Ci, k=3, s=2, p=1, Cin2=Ci2, compact=compact, post_relu=i % 2)
                    lib.alink_debug_set_latency_form(0)
                    base, _, _ = run16(gpu, c, expect=(IGEMM, SELF))
                    check16(base, c, "conv_igemm")
                    lib.alink_debug_set_latency_form(1600)
                    out, _, _ = run16(gpu, c, expect=(IGEMM, LATGEMM))
                    check16(out, c, "latency")
                    assert torch.equal(bits(out), bits(base)), ("conv_gemm_lat_kernel differs from conv_igemm", c.shape, compact)
    finally:
        restore(lib)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_rolling_row_kernels_and_s2c64_shortcut(gpu, dt):
    """The two rolling-row kernels' reports, and conv3x3_s2c64 in its shortcut form with the shortcut's operand on the input
    grid and compact."""
    c = Case(2600, dt, 1, 112, 112, 64, 64, **PRELU_RESID)
    out, _, _ = run16(gpu, c, route=0, expect=(ROLL112, SELF))
    check16(out, c)
    c = Case(2601, dt, 1, 112, 112, 64, 64, s=2, alpha=1, resid=1)
    out, _, _ = run16(gpu, c, route=0, expect=(ROLL112S2, SELF))
    check16(out, c)
    for compact in (0, 1):
        c = Case(2602 + compact, dt, 1, 112, 112, 64, 64, s=2, Cin2=64, compact=compact)
        out, _, _ = run16(gpu, c, route=0, expect=(ROLL112S2, SELF))
        check16(out, c, "shortcut compact=%d" % compact)


def test_refused_requests_return_an_error_and_launch_nothing(gpu):
    lib = gpu.load()
    refused = [
        ("s2c64 shortcut + PReLU", Case(1, "bf16", 1, 112, 112, 64, 64, s=2, Cin2=64, alpha=1), dict(route=0)),
        ("rolling-row + post_relu", Case(2, "bf16", 1, 112, 112, 64, 64, resid=1, post_relu=1), dict(route=0)),
        ("rolling-row + dact", Case(3, "bf16", 1, 112, 112, 64, 64, alpha=1, dact=1), dict(route=0)),
        ("rolling-row + splitk", Case(4, "bf16", 1, 112, 112, 64, 64, s=2), dict(route=0, splitk=3)),
        ("shortcut on a linear-tile layer", Case(5, "bf16", 1, 14, 14, 128, 128, Cin2=64), dict(route=1)),
        ("dact without slopes", Case(6, "bf16", 1, 14, 14, 128, 128, dact=1, reference=False), dict(route=1)),
        ("dact + residual", Case(7, "bf16", 1, 14, 14, 128, 128, alpha=1, dact=1, resid=1), dict(route=1)),
        ("shortcut + splitk", Case(8, "bf16", 1, 14, 14, 128, 128, s=2, Cin2=64), dict(splitk=2)),
        ("splitk no divisor", Case(9, "bf16", 1, 14, 14, 128, 128, s=2), dict(splitk=4)),
    ]
    try:
        for what, c, kw in refused:
            rc, out = run16(gpu, c, rc_only=True, **kw)
            assert rc != 0 and lib.alink_last_error(), what
            assert torch.isnan(out.float()).all(), "%s: refused, but something was written" % what
        # the tile kernels have no K split, no shortcut form
        lib.alink_debug_set_linear(0)
        for what, c, kw in [("tile kernel + splitk", Case(10, "bf16", 2, 13, 14, 128, 256), dict(route=1, splitk=2)),
                            ("tile kernel + shortcut", Case(11, "bf16", 2, 13, 14, 128, 256, Cin2=64), dict(route=1))]:
            rc, out = run16(gpu, c, rc_only=True, **kw)
            assert rc != 0 and lib.alink_last_error(), what
            assert torch.isnan(out.float()).all(), what
        # split precision: no fused shortcut, no backward epilogue (the 16-bit entry does not take the type at all)
        c = Case(12, "bf16", 1, 14, 14, 128, 128, s=2, Cin2=64)
        d = c.cuda()
        out = torch.full((1, 7, 7, 128), float("nan"), dtype=torch.float32, device="cuda")
        rc = lib.alink_conv_nhwc_ex(gpu.DT_F16X2, gpu.ptr(d["x"]), gpu.ptr(d["w"]), gpu.ptr(d["bias"]), None, None, gpu.ptr(out),
                                    1, 14, 14, 128, 128, 3, 2, 1, 0, -1, 0, None, 0, gpu.ptr(d["in2"]), gpu.ptr(d["w2"]), 64, 0, 1,
                                    None, None, None)
        assert rc != 0 and lib.alink_last_error() and torch.isnan(out).all()
        # split precision: a K split that would cut inside a real K-step's three products
        x = Case(13, "x2", 1, 8, 8, 128, 64, k=1, s=1, p=0)
        rc, out = runx2(gpu, x, splitk=3, rc_only=True)
        assert rc != 0 and lib.alink_last_error() and torch.isnan(out).all()
    finally:
        restore(lib)


# ---- post_relu keeps a NaN (alink_backbone_range_flag rests on it) --------------------------------------------------------------
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_post_relu_keeps_a_nan(gpu, dt):
    lib = gpu.load()
    families = [
        # name, shape, switches, route, expected report
        ("linear", (2, 7, 7, 128, 128, 3, 1, 1), dict(latency=0), 1, (LIN7, SELF)),
        ("latency 3x3", (2, 7, 7, 128, 128, 3, 1, 1), dict(), 1, (LIN7, LAT3X3)),
        ("tile", (2, 13, 14, 64, 256, 3, 1, 1), dict(linear=0, pair=0), 1, (D1, SELF)),
        ("pair", (2, 13, 14, 64, 256, 3, 1, 1), dict(linear=0), 1, (S1, SELF)),
        ("gemm", (2, 14, 14, 128, 128, 1, 2, 0), dict(latency=0), 0, (IGEMM, SELF)),
        ("latency gemm", (2, 14, 14, 128, 128, 1, 2, 0), dict(), 0, (IGEMM, LATGEMM)),
        ("split finish", (2, 7, 7, 128, 128, 3, 1, 1), dict(latency=0, splitk=2), 1, (LIN7, SELF)),
    ]
    try:
        for name, shp, sw, route, expect in families:
            restore(lib)
            if "latency" in sw: lib.alink_debug_set_latency_form(sw["latency"])
            if "linear" in sw: lib.alink_debug_set_linear(sw["linear"])
            if "pair" in sw: lib.alink_debug_set_pair(sw["pair"])
            Ho, Wo = _out_hw(shp[1], shp[2], shp[5], shp[6], shp[7])
            at = (shp[0] * Ho * Wo * shp[4]) // 2 + 37
            c = Case(2700, dt, *shp[:5], k=shp[5], s=shp[6], p=shp[7], resid=1, post_relu=1, nan_at=at)
            out, _, _ = run16(gpu, c, route=route, splitk=sw.get("splitk", 1), expect=expect)
            got = out.float().cpu().view(-1)
            nan = torch.isnan(got)
            assert nan[at] and int(nan.sum()) == 1, "%s: NaN at %s, wanted exactly [%d]" % (name, nan.nonzero().view(-1).tolist()[:8], at)
            assert torch.isfinite(got[~nan]).all(), name
    finally:
        restore(lib)


# ---- split precision ------------------------------------------------------------------------------------------------------------
def runx2(gpu, c, fine=-1, nprod=3, splitk=1, expect=None, rc_only=False, exps=(9, 14, 8, 10)):
    lib = gpu.load()
    N, H, W, Ci, Co, k, s, p = c.shape
    d = c.cuda()
    out = torch.full((N, c.Ho, c.Wo, Co), float("nan"), dtype=torch.float32, device="cuda")
    kern, form = C.c_int(-7), C.c_int(-7)
    rc = lib.alink_conv_nhwc_x2_ex(gpu.ptr(d["x"]), gpu.ptr(d["w"]), gpu.ptr(d["bias"]), gpu.ptr(d["alpha"]), gpu.ptr(d["resid"]),
                                   gpu.ptr(out), N, H, W, Ci, Co, k, s, p, c.flags["border"], fine, exps[0], exps[1], exps[2], exps[3],
                                   nprod, splitk, c.flags["post_relu"], C.byref(kern), C.byref(form), None)
    if rc_only:
        return rc, out
    gpu.check(rc, "alink_conv_nhwc_x2_ex %s" % (c.shape,))
    if expect is not None:
        assert (kern.value, form.value) == expect, "case %s: ran kernel %d form %d, written for %s" % (c.shape, kern.value, form.value, expect)
    return out


def checkx2(out, c, nprod, what=""):
    got = out.cpu()
    assert torch.isfinite(got).all(), (c.shape, what)
    err = ((got.double() - c.ref).abs() / c.mag).max().item()
    print("x2 %s %s nprod=%d %s: err / sum|products| = %.3g" % (c.shape, c.flags, nprod, what, err))
    assert err < (4e-6 if nprod == 3 else 1.0e-3), (c.shape, what, nprod, err)


X2_CASES = [
    # shape (N, H, W, Cin, Cout, ksz, stride, pad), epilogue, kernel, has a latency form, K splits to run (latency form off)
    ((1, 112, 112, 64, 64, 3, 1, 1), PRELU, LIN112, None, ()),
    ((1, 56, 56, 64, 64, 3, 1, 1), RESID_RELU, LIN56, None, ()),
    ((3, 7, 7, 128, 128, 3, 1, 1), PRELU_RESID, LIN7, LAT3X3, (2,)),                 # 147 pixels
    ((1, 14, 14, 256, 128, 3, 1, 1), RESID_RELU, LIN14, LAT3X3, (2, 4)),
    ((1, 28, 28, 128, 128, 3, 1, 1), PRELU, LIN28, LAT3X3, ()),
    ((2, 14, 14, 128, 128, 3, 2, 1), RESID, IGEMM, LATGEMM, (2, 3)),                 # 18 real K-steps: 9 / 6 per split, x 3 products
    ((3, 8, 8, 64, 128, 1, 2, 0), dict(alpha=1), IGEMM, LATGEMM, ()),
    ((2, 14, 14, 256, 64, 1, 1, 0), RESID_RELU, IGEMM, LATGEMM, (2,)),
]


@pytest.mark.parametrize("case", range(len(X2_CASES)))
def test_split_precision_forms(gpu, case):
    """Both product counts on every split-precision kernel and form: three products to 4e-6 of sum|products|, one product to
    1e-3 and NOT equal to the three-product result (the flag is honoured); latency forms bit-equal to the kernels proper;
    K splits; the 64-channel form bit-equal to the 128-channel one."""
    lib = gpu.load()
    shp, epi, kern, lat, splits = X2_CASES[case]
    c = Case(2800 + case, "x2", *shp[:5], k=shp[5], s=shp[6], p=shp[7], **epi)
    try:
        res = {}
        for nprod in (3, 1):
            lib.alink_debug_set_latency_form(0)
            fines = (0, 1) if kern in (LIN7, LIN14, LIN28) else (-1,)
            for fine in fines:
                out = runx2(gpu, c, fine=fine, nprod=nprod, expect=(kern, SELF))
                checkx2(out, c, nprod, "fine=%d" % fine)
                if fine != fines[0]:
                    assert torch.equal(bits(out), bits(res[nprod])), ("the 64-channel form changed a bit", shp, nprod)
                else:
                    res[nprod] = out
            for S in splits:
                out = runx2(gpu, c, fine=fines[0], nprod=nprod, splitk=S, expect=(kern, SELF))
                checkx2(out, c, nprod, "splitk=%d" % S)
            if lat is not None:
                lib.alink_debug_set_latency_form(1600)
                for tiles in ((0, 1, 2) if lat == LAT3X3 else (-1,)):
                    lib.alink_debug_set_latency_tiles(tiles)
                    out = runx2(gpu, c, nprod=nprod, expect=(kern, lat))
                    checkx2(out, c, nprod, "latency tiles=%d" % tiles)
                    assert torch.equal(bits(out), bits(res[nprod])), ("latency form differs from the kernel proper", shp, nprod, tiles)
                lib.alink_debug_set_latency_tiles(-1)
        assert not torch.equal(res[1], res[3]), "nprod = 1 gave the three-product result: the flag is not honoured"
    finally:
        restore(lib)
