"""Cases and float64 references for the exact-f32 GEMM (a-link_amd/csrc/sgemm.hip), shared by tests/test_gpu_gemm32.py (which
runs them through alink_gemm32_ex) and tests/test_gemm32_cases.py (which checks, without a device, that they are what they claim).

A case holds the operand STORAGE exactly as the kernel is handed it (padded rows, transposed layouts, NHWC tensors in one or
two buffers) and the launch request.  The reference never follows the kernel's indexing: plain modes are a matmul on explicitly
transposed slices of that storage, the convolution modes are torch's conv2d / its autograd in float64.

EXACT cases use small integers (operands -8 .. 8, pixels 0 .. 255 under a pre-scaling of 2^-7 steps, PReLU slopes 0.25 / 0.5):
every product and every partial sum, in any order, is a multiple of one power of two below 2^24 of them — representable in
float32 — so the kernel's result must equal the float64 reference bit for bit whatever the tile, stage depth, loader form or
split.  REAL cases (randn) are held to the worst-case bound of a float32 accumulation instead."""
import zlib

import torch
import torch.nn.functional as F

A_ROW, A_COL, A_CONV, A_CONVT = 0, 1, 2, 3
B_ROW, B_COLT, B_FLIP = 0, 1, 2
PAIRS = [(A_ROW, B_ROW), (A_ROW, B_COLT), (A_COL, B_ROW), (A_CONV, B_ROW), (A_CONV, B_FLIP), (A_CONVT, B_ROW)]
PAIR_NAME = {(A_ROW, B_ROW): "row-row", (A_ROW, B_COLT): "row-colt", (A_COL, B_ROW): "col-row", (A_CONV, B_ROW): "conv-row",
             (A_CONV, B_FLIP): "conv-flip", (A_CONVT, B_ROW): "convt-row"}
# every kernel instantiation the launcher can reach: (amode, bmode, tile columns, stage depth, 16-byte loaders)
ALL_FORMS = [(a, b, t, s, v) for (a, b) in PAIRS for t in (32, 64) for s in (16, 64) for v in (0, 1)]

EPILOGUE_TERMS = ("bias", "alpha", "relu", "act", "resid", "accumulate")


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(g, *shape, lo=-8, hi=8, zeros=0.06):
    """integers lo .. hi, mostly non-zero"""
    t = torch.randint(lo, hi + 1, shape, generator=g).float()
    t[t == 0] = 1.0
    t[torch.rand(shape, generator=g) < zeros] = 0.0
    return t


def out_hw(H, W, ks, stride, pad):
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


class Case:
    """One launch request.  Storage tensors are float32 on the CPU:
       a_parts   plain: [one 2-D (rows, lda)]; conv modes: one or two NHWC tensors (the second = GemmP::A2, a_split = images in the first)
       b_store   2-D (rows, ldb) for B_ROW / B_COLT; (3, 3, N, Ci) for B_FLIP
       bias, alpha (N,); act, resid, oldc (M, N) — the runner stores them with pitch ldc — or None
       plan      max_split >= 1: the planner; 0: the caller's splitk / kper
       a_off / b_off   the operand's base is moved by this many floats (1: no 16-byte alignment)
       expect    (tile, stage, vec) this case was written for; split = (splitk, kper) where the case pins the plan too"""

    def __init__(self, name, kind, amode, bmode, M, N, K, a_parts, b_store, lda=0, ldb=0, ldc=None, geom=None, exact=True,
                 bias=None, alpha=None, act=None, resid=None, oldc=None, relu=0, max_split=1, splitk=1, kper=0, force_bk=0,
                 a_off=0, b_off=0, expect=None, split=None):
        self.name, self.kind, self.amode, self.bmode = name, kind, amode, bmode
        self.M, self.N, self.K, self.lda, self.ldb = M, N, K, lda, ldb
        self.a_parts, self.b_store = a_parts, b_store
        self.geom = dict(H=0, W=0, Ci=0, Ho=0, Wo=0, pad=0, prescale=0, ks=0, cstride=0, pre_sub=0.0, pre_mul=0.0)
        self.geom.update(geom or {})
        self.exact = exact
        self.bias, self.alpha, self.act, self.resid, self.oldc, self.relu = bias, alpha, act, resid, oldc, relu
        self.accumulate = 0 if oldc is None else 1
        self.max_split, self.splitk, self.kper, self.force_bk = max_split, splitk, kper, force_bk
        self.a_off, self.b_off = a_off, b_off
        self.ldc = ldc if ldc is not None else N
        self.expect = expect if expect is not None else form_of(self)
        self.split = split
        self._ref = None

    @property
    def a_split(self):
        return self.a_parts[0].shape[0] if len(self.a_parts) > 1 else 0

    @property
    def form(self):
        return (self.amode, self.bmode) + tuple(self.expect)

    def reference(self):
        """float64 (M, N), computed once and shared"""
        if self._ref is None:
            self._ref = epilogue(self, linear(self, torch.float64), torch.float64)
        return self._ref


# ---- what the launcher is documented to choose (sgemm.hip: narrow(), deep(), vec_ok(), launch_t) -------------------------------
def form_of(c):
    """(tile, stage, vec) by the launcher's documented rules, for cases that do not state the form by hand.  Every case here is
    tiny (tiles x slabs far below deep()'s 512), so the grid's part of deep() is always true."""
    tile = 32 if c.N <= 32 else 64
    planned = c.max_split >= 1
    whole = planned or c.kper % 64 == 0                          # the planner's kper is a multiple of 64
    want_deep = c.force_bk == 64 if c.force_bk else c.K >= 24
    stage = 64 if (want_deep and whole) else 16
    g = c.geom
    if c.amode == A_ROW:
        a = c.K % 4 == 0 and c.lda % 4 == 0
    elif c.amode == A_COL:
        a = c.M % 4 == 0 and c.lda % 4 == 0
    elif c.amode == A_CONV:
        a = g["Ci"] % 4 == 0 and g["prescale"] == 0
    else:
        a = g["Ci"] % 4 == 0 and 2 * g["Wo"] >= (8 if tile == 32 else 16) and len(c.a_parts) == 1
    if c.bmode == B_ROW:
        b = c.N % 4 == 0 and c.ldb % 4 == 0
    elif c.bmode == B_COLT:
        b = c.K % 4 == 0 and c.ldb % 4 == 0
    else:
        b = True
    return (tile, stage, int(a and b and c.a_off % 4 == 0 and c.b_off % 4 == 0))


# ---- references ----------------------------------------------------------------------------------------------------------------
def prescaled(c, x):
    p = c.geom["prescale"]
    if p == 1:
        return (x - 128.0) / 128.0                               # SmallRes.preprocess
    if p == 2:
        return (x - c.geom["pre_sub"]) * c.geom["pre_mul"]
    return x


def linear(c, dtype, absolute=False):
    """A . B of the case in `dtype`, (M, N); absolute: of |A| and |B| (the sum of |products|)"""
    f = (lambda t: t.abs()) if absolute else (lambda t: t)
    M, N, K, g = c.M, c.N, c.K, c.geom
    if c.kind == "plain":
        a = c.a_parts[0].to(dtype)
        a = a[:, :K] if c.amode == A_ROW else a[:, :M].t()       # A_COL: stored [K][M]
        b = c.b_store.to(dtype)
        b = b[:, :N] if c.bmode == B_ROW else b[:, :K].t()       # B_COLT: stored [N][K]
        assert a.shape == (M, K) and b.shape == (K, N)
        return f(a) @ f(b)
    x = f(prescaled(c, torch.cat(c.a_parts, 0).to(dtype))).permute(0, 3, 1, 2)          # NCHW
    if c.kind == "conv":                                         # weights (ky, kx, ci, co) row-major = [K][N]
        ks, s = g["ks"] or 3, g["cstride"] or 1
        w = c.b_store.to(dtype)[:, :N].reshape(ks, ks, g["Ci"], N).permute(3, 2, 0, 1)
        y = F.conv2d(x, f(w), stride=s, padding=g["pad"])
        assert y.shape[2:] == (g["Ho"], g["Wo"])
        return y.permute(0, 2, 3, 1).reshape(M, N)
    if c.kind == "dgrad":                                        # x is dz (n, Co, Hz, Wz); the layer: N -> Co channels, padding 2 - pad
        w = c.b_store.to(dtype).permute(3, 2, 0, 1)              # (ky, kx, ci, co) -> (co, ci, ky, kx)
        xin = torch.zeros(x.shape[0], N, g["Ho"], g["Wo"], dtype=dtype, requires_grad=True)
        z = F.conv2d(xin, f(w), padding=2 - g["pad"])
        assert z.shape == x.shape
        z.backward(x.contiguous())
        return xin.grad.permute(0, 2, 3, 1).reshape(M, N)
    assert c.kind == "wgrad"                                     # B = dz (pixels, N); rows (ky, kx, ci), then the bias gradient
    Ci = g["Ci"]
    dz = f(c.b_store.to(dtype)[:, :N]).reshape(x.shape[0], g["Ho"], g["Wo"], N).permute(0, 3, 1, 2)
    w0 = torch.zeros(N, Ci, 3, 3, dtype=dtype, requires_grad=True)
    b0 = torch.zeros(N, dtype=dtype, requires_grad=True)
    z = F.conv2d(x, w0, b0, padding=g["pad"])
    assert z.shape == dz.shape
    z.backward(dz.contiguous())
    return torch.cat([w0.grad.permute(2, 3, 1, 0).reshape(9 * Ci, N), b0.grad[None, :]], 0)


def epilogue(c, v, dtype):
    """the kernel's order: bias, PReLU, ReLU, act mask, residual, accumulate"""
    if c.bias is not None:
        v = v + c.bias.to(dtype)
    if c.alpha is not None:
        v = torch.where(v > 0, v, v * c.alpha.to(dtype))
    if c.relu:
        v = torch.clamp_min(v, 0.0)
    if c.act is not None:
        v = torch.where(c.act > 0, v, torch.zeros((), dtype=dtype))
    if c.resid is not None:
        v = v + c.resid.to(dtype)
    if c.oldc is not None:
        v = v + c.oldc.to(dtype)
    return v


def magnitude(c):
    """sum |a||b| + |bias| + |resid| + |old C| per output, float64"""
    m = linear(c, torch.float64, absolute=True)
    for t in (c.bias, c.resid, c.oldc):
        if t is not None:
            m = m + t.double().abs()
    return m


def unit(c):
    """the smallest step of an exact case's results: operand steps multiplied"""
    u = {0: 1.0, 1: 2.0 ** -7, 2: 2.0 ** -8}[c.geom["prescale"]]
    return u * (0.25 if c.alpha is not None else 1.0)


# ---- builders ------------------------------------------------------------------------------------------------------------------
def epi_terms(g, M, N, terms, exact=True):
    """the epilogue operands named in `terms` (integers, or randn for a real-valued case)"""
    draw = (lambda *s: ints(g, *s, lo=-9, hi=9)) if exact else (lambda *s: torch.randn(*s, generator=g))
    kw = {}
    if "bias" in terms:
        kw["bias"] = draw(N)
    if "alpha" in terms:
        kw["alpha"] = torch.tensor([0.25, 0.5])[torch.randint(0, 2, (N,), generator=g)]
    if "relu" in terms:
        kw["relu"] = 1
    if "act" in terms:
        a = torch.randn(M, N, generator=g)
        flat = a.view(-1)
        flat[::5] = 0.0                                          # exact zeros of both signs: masked like the negatives
        flat[3::7] = -0.0
        kw["act"] = a
    if "resid" in terms:
        kw["resid"] = draw(M, N)
    if "accumulate" in terms:
        kw["oldc"] = draw(M, N)
    return kw


def _padded(t, ld):
    """rows of t in a (rows, ld) store whose padding is NaN: a padded value that reaches a product shows"""
    s = torch.full((t.shape[0], ld), float("nan"))
    s[:, :t.shape[1]] = t
    return s


def plain(name, amode, bmode, M, N, K, lda_pad=0, ldb_pad=0, terms=(), exact=True, **kw):
    g = _gen(name)
    draw = (lambda *s: ints(g, *s)) if exact else (lambda *s: torch.randn(*s, generator=g))
    a, b = draw(M, K), draw(K, N)
    a_st = a if amode == A_ROW else a.t().contiguous()           # explicit transposes: the reference undoes them by slicing
    b_st = b if bmode == B_ROW else b.t().contiguous()
    lda, ldb = a_st.shape[1] + lda_pad, b_st.shape[1] + ldb_pad
    kw.setdefault("ldc", N + 3)
    return Case(name, "plain", amode, bmode, M, N, K, [_padded(a_st, lda)], _padded(b_st, ldb), lda=lda, ldb=ldb, exact=exact,
                **epi_terms(g, M, N, terms, exact), **kw)


def _images(g, n, H, W, Ci, prescale, exact):
    if prescale:
        return torch.randint(0, 256, (n, H, W, Ci), generator=g).float()
    return ints(g, n, H, W, Ci) if exact else torch.randn(n, H, W, Ci, generator=g)


def _parts(x, n2):
    return [x] if not n2 else [x[:x.shape[0] - n2].contiguous(), x[x.shape[0] - n2:].contiguous()]


def _geom(H, W, Ci, Ho, Wo, pad, prescale, ks=0, cstride=0):
    g = dict(H=H, W=W, Ci=Ci, Ho=Ho, Wo=Wo, pad=pad, prescale=prescale, ks=ks, cstride=cstride)
    if prescale == 2:
        g.update(pre_sub=127.5, pre_mul=0.0078125)               # the float32 backbone's (x - 127.5) / 128
    return g


def conv(name, n, H, W, Ci, N, ks=3, stride=1, pad=1, prescale=0, n2=0, ldb_pad=0, terms=(), exact=True, explicit=True, **kw):
    """A_CONV + B_ROW: n images (the last n2 of them in the second buffer); explicit: ks / cstride spelled out, else the defaults 0"""
    g = _gen(name)
    Ho, Wo = out_hw(H, W, ks, stride, pad)
    M, K = n * Ho * Wo, ks * ks * Ci
    x = _images(g, n, H, W, Ci, prescale, exact)
    w = ints(g, K, N) if exact else torch.randn(K, N, generator=g)
    geom = _geom(H, W, Ci, Ho, Wo, pad, prescale, ks if explicit else 0, stride if explicit else 0)
    kw.setdefault("ldc", N + 3)
    return Case(name, "conv", A_CONV, B_ROW, M, N, K, _parts(x, n2), _padded(w, N + ldb_pad), ldb=N + ldb_pad, geom=geom,
                exact=exact, **epi_terms(g, M, N, terms, exact), **kw)


def dgrad(name, n, H, W, Co, N, pad, terms=(), exact=True, **kw):
    """A_CONV + B_FLIP: the input gradient (n, H, W, N) of a 3x3 layer N -> Co channels with padding 2 - pad, from its dz"""
    g = _gen(name)
    fpad = 2 - pad
    Hz, Wz = out_hw(H, W, 3, 1, fpad)
    draw = (lambda *s: ints(g, *s)) if exact else (lambda *s: torch.randn(*s, generator=g))
    dz, w = draw(n, Hz, Wz, Co), draw(3, 3, N, Co)
    M = n * H * W
    kw.setdefault("ldc", N + 3)
    return Case(name, "dgrad", A_CONV, B_FLIP, M, N, 9 * Co, [dz], w, geom=_geom(Hz, Wz, Co, H, W, pad, 0), exact=exact,
                **epi_terms(g, M, N, terms, exact), **kw)


def wgrad(name, n, Ho, Wo, Ci, N, pad, prescale=0, n2=0, ldb_pad=0, terms=(), exact=True, **kw):
    """A_CONVT + B_ROW: weight and bias gradient (9 Ci + 1, N) of a 3x3 layer from its input and dz (n, Ho, Wo, N)"""
    g = _gen(name)
    H, W = Ho + 2 - 2 * pad, Wo + 2 - 2 * pad
    x = _images(g, n, H, W, Ci, prescale, exact)
    K, M = n * Ho * Wo, 9 * Ci + 1
    dz = ints(g, K, N) if exact else torch.randn(K, N, generator=g)
    kw.setdefault("ldc", N + 3)
    return Case(name, "wgrad", A_CONVT, B_ROW, M, N, K, _parts(x, n2), _padded(dz, N + ldb_pad), ldb=N + ldb_pad,
                geom=_geom(H, W, Ci, Ho, Wo, pad, prescale), exact=exact, **epi_terms(g, M, N, terms, exact), **kw)


def fixed(splitk, kper, force_bk=0):
    """the caller-fixed plan (max_split = 0), as alink_smallres_score_pairs and the float32 backbone's FC launch"""
    return dict(max_split=0, splitk=splitk, kper=kper, force_bk=force_bk, ldc=None)


# ---- the exact cases, by group (one parametrised GPU test per group) -----------------------------------------------------------
GROUPS = {}


def _add(group, case):
    assert case.exact
    GROUPS.setdefault(group, []).append(case)
    return case


def _build_plain():
    # every (M, N, K) of the issue's lists for the three plain pairs: K shorter than a stage (4), an odd tail (17), 28, exactly
    # one deep stage (64), one stage + 1 (65), a partial last slab (200); M = 1, one short of / one past a 64-row tile, one past
    # a 128-row tile; N at and around the 32-column tile.  Stage depth and row pitch rotate through the combinations.
    for am, bm in PAIRS[:3]:
        for M in (1, 63, 65, 129) + ((68,) if am == A_COL else ()):      # (A_COL: 16-byte loads need M % 4 == 0)
            i = 0
            for N in (8, 32, 33, 100):
                for K in (4, 17, 28, 64, 65, 200):
                    i += 1
                    force = (0, 16, 64)[i % 3]
                    lda_pad, ldb_pad = (0, 4, 0, 5)[i % 4], (0, 0, 8, 3)[(i // 2) % 4]      # tight, padded by whole quads, odd
                    _add("plain/%s/M%d" % (PAIR_NAME[am, bm], M),
                         plain("plain-%s-%dx%dx%d" % (PAIR_NAME[am, bm], M, N, K), am, bm, M, N, K, lda_pad, ldb_pad,
                               force_bk=force))


def _build_conv():
    # non-square 5 x 7 maps, two images (M = 70 or 24: no multiple of either tile; 70 rows = two 64-row tiles)
    geoms = {"3x3p1": (3, 1, 1), "3x3p0": (3, 1, 0), "3x3s2p1": (3, 2, 1), "1x1s1": (1, 1, 0), "1x1s2": (1, 2, 0)}
    cis = [(3, 1), (3, 2), (4, 0), (12, 0), (20, 0), (32, 0)]    # (Ci, prescale); 12 and 20: ci_magic on a non-power of two
    for gi, (gname, (ks, s, pad)) in enumerate(geoms.items()):
        for ci_i, (Ci, pre) in enumerate(cis):
            j = gi + ci_i
            N = (8, 40, 33, 32, 100)[j % 5]
            _add("conv/" + gname, conv("conv-%s-ci%d-p%d-n%d" % (gname, Ci, pre, N), 2, 5, 7, Ci, N, ks, s, pad, pre,
                                       ldb_pad=(0, 4)[j % 2], force_bk=(0, 16, 64)[j % 3],
                                       terms=[(), ("bias", "relu"), ("bias", "alpha", "resid")][j % 3],
                                       explicit=not (ks == 3 and s == 1 and j % 2)))       # SmallRes leaves ks / cstride 0
    # two buffers: 3 + 2 images of 5 x 5, rows 75 .. 124 come from the second — inside the 64-row tile 64 .. 127 and the one 128-row tile
    for Ci, pre, N in [(4, 0, 40), (4, 0, 32), (3, 1, 40), (3, 1, 8), (20, 0, 64)]:
        for force in (16, 64):
            _add("conv/two-buffers", conv("conv-a2-ci%d-n%d-bk%d" % (Ci, N, force), 5, 5, 5, Ci, N, 3, 1, 1, pre, n2=2,
                                          force_bk=force, terms=("bias", "relu")))
    # a K split of the gather (SmallRes' small batches: max_split 4 once K >= 512): Ci = 64, K = 576 -> 3 slabs of 192
    _add("conv/two-buffers", conv("conv-split-ci64", 2, 5, 7, 64, 32, 3, 1, 0, max_split=4, ldc=None, terms=("bias", "relu"),
                                  split=(3, 192)))
    _add("conv/two-buffers", conv("conv-a2-split-ci64", 5, 5, 5, 64, 64, 3, 1, 1, n2=2, max_split=4, ldc=None,
                                  terms=("bias", "relu"), split=(3, 192)))


def _build_dgrad():
    for pad in (1, 2):                                           # 2: the layer had no padding, the gradient map is larger than dz
        i = 0
        for Co in (4, 12, 32):
            for N in (4, 12, 32, 64):
                i += 1
                _add("dgrad/pad%d" % pad, dgrad("dgrad-p%d-co%d-n%d" % (pad, Co, N), 2, 5, 7, Co, N, pad,
                                                terms=("act",) if i % 2 else (), force_bk=(0, 16, 64)[i % 3],
                                                a_off=1 if i % 4 == 0 else 0))
        # both stage depths, aligned and not, on both tiles
        for Co in (4, 32):
            for N in (12, 64):
                for bk in (16, 64):
                    for off in (0, 1):
                        _add("dgrad/pad%d" % pad, dgrad("dgrad-p%d-co%d-n%d-bk%d-off%d" % (pad, Co, N, bk, off), 3, 4, 6, Co, N, pad,
                                                        terms=("act",) if off else (), force_bk=bk, a_off=off))
        # split along K: dz channels 64 -> K = 576, three slabs; the act mask then applies in the slab sum
        _add("dgrad/pad%d" % pad, dgrad("dgrad-p%d-split" % pad, 2, 5, 7, 64, 32, pad, terms=("act",), max_split=4, ldc=None,
                                        split=(3, 192)))


def _build_wgrad():
    W = lambda *a, **k: _add("wgrad/" + a[0].split("-")[1], wgrad(*a, **k))
    # the three channel counts: Ci = 3 pre-scaled (M = 28, 4-byte), 4 (M = 37), 32 (M = 289: the ones row alone in the last tile)
    for pad in (0, 1):
        for N in (32, 64):
            W("wgrad-ci-3-p%d-n%d" % (pad, N), 3, 4, 9, 3, N, pad, prescale=1)
            W("wgrad-ci-4-p%d-n%d" % (pad, N), 3, 4, 9, 4, N, pad)
            W("wgrad-ci-32-p%d-n%d" % (pad, N), 3, 4, 9, 32, N, pad, force_bk=(16, 64)[pad])
    # the carried pixel walk at its limits.  64 x 64 tile: a thread steps 16 pixels — two rows of Wo = 8, and with Ho = 1 or 2
    # one or two images; 128 x 32 tile: 8 pixels — two rows and two images of Wo = 4, Ho = 1.  Both stage depths, both pads.
    for pad in (0, 1):
        for bk in (16, 64):
            for Ho in (1, 2):
                W("wgrad-walk-wo8-ho%d-p%d-bk%d" % (Ho, pad, bk), 9, Ho, 8, 4, 64, pad, force_bk=bk, expect=(64, bk, 1))
            W("wgrad-walk-wo4-ho1-p%d-bk%d" % (pad, bk), 19, 1, 4, 4, 32, pad, force_bk=bk, expect=(32, bk, 1))
            W("wgrad-walk-wo4-ho3-p%d-bk%d" % (pad, bk), 7, 3, 4, 8, 8, pad, force_bk=bk, expect=(32, bk, 1))
            # rows too short for the walk on the wide tile: the launcher must fall back to the 4-byte form
            W("wgrad-walk-wo7-p%d-bk%d" % (pad, bk), 3, 5, 7, 4, 64, pad, force_bk=bk, expect=(64, bk, 0))
            # Wo = 10, Ho = 5 under a caller-fixed K split: slabs begin at pixel 16 / 64 — row 1, columns 6 / 4 — and 128 — image 2, row 2
            W("wgrad-walk-wo10-split-p%d-bk%d" % (pad, bk), 3, 5, 10, 4, 64, pad, expect=(64, bk, 1),
              **fixed(150 // bk + 1, bk, bk))
        W("wgrad-walk-wo10-narrow-split-p%d" % pad, 3, 5, 10, 12, 32, pad, expect=(32, 64, 1), **fixed(3, 64, 64))
    # pre-scaling in the 16-byte form (Ci = 4: no production layer has it), both kinds of scaling, both tiles
    for pre in (1, 2):
        for N in (32, 64):
            W("wgrad-prescale-ci4-pre%d-n%d" % (pre, N), 2, 4, 9, 4, N, 1, prescale=pre, expect=(N, 64, 1))
    W("wgrad-prescale-ci4-split", 3, 5, 10, 4, 64, 1, prescale=1, expect=(64, 16, 1), **fixed(10, 16))
    # two buffers (the two sides of a siamese batch): always the 4-byte form
    for Ci, pre in [(4, 0), (3, 1), (32, 0)]:
        for N in (32, 64):
            W("wgrad-a2-ci%d-n%d" % (Ci, N), 5, 3, 8, Ci, N, 1, prescale=pre, n2=2, force_bk=(64, 16)[N == 32])
    W("wgrad-a2-split", 5, 3, 8, 4, 64, 1, n2=2, **fixed(2, 64))
    # accumulate (the second siamese branch of conv1), in the kernel and in the slab sum
    for Ci, pre in [(4, 0), (3, 1)]:
        W("wgrad-accumulate-ci%d" % Ci, 3, 4, 9, Ci, 32, 1, prescale=pre, terms=("accumulate",))
        W("wgrad-accumulate-ci%d-split" % Ci, 3, 4, 9, Ci, 32, 1, prescale=pre, terms=("accumulate",), **fixed(2, 64))
        W("wgrad-accumulate-ci%d-planned" % Ci, 7, 6, 9, Ci, 64, 1, prescale=pre, terms=("accumulate",), max_split=128, ldc=None,
          split=(2, 192))


def _build_epilogue():
    # each term alone and all together; every case unsplit (the kernel's epilogue) and split (splitk_reduce_kernel's copy), on
    # both tiles — each must equal the reference, and so each other
    # (two pairs whose ORDER shows: PReLU after the bias, the residual after the act mask)
    for terms in [(t,) for t in EPILOGUE_TERMS] + [("bias", "alpha"), ("act", "resid"), EPILOGUE_TERMS]:
        tag = "all" if len(terms) > 2 else "-".join(terms)
        for N in (8, 33):
            _add("epilogue/" + tag, plain("epi-%s-n%d" % (tag, N), A_ROW, B_ROW, 65, N, 200, terms=terms))
            _add("epilogue/" + tag, plain("epi-%s-n%d-split" % (tag, N), A_ROW, B_ROW, 65, N, 200, terms=terms, **fixed(4, 64)))
        _add("epilogue/" + tag, plain("epi-%s-planned-split" % tag, A_ROW, B_ROW, 65, 33, 520, terms=terms, max_split=8, ldc=None,
                                      split=(3, 192)))


def _build_slabs():
    # more than one slab per group of the slab sum (it adds slabs g, g + 8, ...), uneven groups; M N = 33: a last block of one
    for M, N in [(1, 33), (33, 1), (3, 11)]:
        for S in (2, 8, 9, 17):
            _add("slabs/fixed", plain("slabs-%dx%d-s%d" % (M, N, S), A_ROW, B_ROW, M, N, 16 * S - 5, lda_pad=1,
                                      split=(S, 16), **fixed(S, 16)))
    _add("slabs/fixed", plain("slabs-65x33-s17-deep", A_ROW, B_ROW, 65, 33, 64 * 17 - 9, split=(17, 64), **fixed(17, 64, 64)))
    # kper a multiple of 16 but not of 64: stage 16 even where the caller asks for 64
    _add("slabs/fixed", plain("slabs-kper48-force64", A_ROW, B_ROW, 65, 36, 200, expect=(64, 16, 1), split=(5, 48),
                              **fixed(5, 48, 64)))
    _add("slabs/fixed", plain("slabs-kper48-colt", A_ROW, B_COLT, 65, 8, 200, expect=(32, 16, 1), split=(5, 48), **fixed(5, 48, 64)))
    _add("slabs/fixed", plain("slabs-kper80-col", A_COL, B_ROW, 68, 100, 200, expect=(64, 16, 1), split=(3, 80), **fixed(3, 80)))
    # the planner: powers of two while a slab keeps two deep stages; kper a multiple of 64
    for (M, N), K, ms, split in [((1, 33), 512, 2, (2, 256)), ((3, 11), 1024, 8, (8, 128)), ((33, 1), 1100, 8, (6, 192)),
                                 ((65, 100), 2112, 128, (11, 192)), ((129, 32), 8192, 128, (64, 128))]:
        _add("slabs/planned", plain("slabs-planned-%dx%dx%d" % (M, N, K), A_ROW, B_ROW, M, N, K, max_split=ms, ldc=None, split=split))
    _add("slabs/planned", plain("slabs-planned-colt", A_ROW, B_COLT, 63, 33, 1024, max_split=4, ldc=None, split=(4, 256)))
    _add("slabs/planned", plain("slabs-planned-col", A_COL, B_ROW, 68, 32, 520, max_split=16, ldc=None, split=(3, 192)))


def _pin_case(am, bm, tile, stage, vec):
    """the case written to reach one instantiation: small, more than one tile along M, the stage depth through deep() where
    the reduction length allows and through force_bk otherwise"""
    name = "pin-%s-t%d-s%d-v%d" % (PAIR_NAME[am, bm], tile, stage, vec)
    N = 32 if tile == 32 else 64
    if (am, bm) in PAIRS[:3]:
        # 16-byte form: every dimension and pitch a multiple of 4; 4-byte form: K = 17 (row modes), M = 133 (A_COL)
        K = 28 if (vec or am == A_COL) else 17
        M = 132 if (vec or am != A_COL) else 133
        by_deep = (K >= 24) == (stage == 64)                     # deep() itself gives the wanted depth
        return plain(name, am, bm, M, N, K, lda_pad=4, ldb_pad=4, force_bk=0 if by_deep else stage, expect=(tile, stage, vec))
    if (am, bm) == (A_CONV, B_ROW):
        # stage 16 through deep(): a 1x1 layer with K = Ci = 4 (16-byte) or 3 (4-byte); stage 64 through deep(): 3x3, K = 36 / 27
        ks = 1 if stage == 16 else 3
        return conv(name, 3, 5, 7, 4 if vec else 3, N, ks, 1, ks // 2, prescale=0 if vec else 2, expect=(tile, stage, vec))
    if (am, bm) == (A_CONV, B_FLIP):
        # K = 36 >= 24: deep() gives 64; the 4-byte form only through a dz base that is not 16-byte aligned
        return dgrad(name, 3, 5, 7, 4, N, 1, terms=("act",), force_bk=0 if stage == 64 else 16, a_off=0 if vec else 1,
                     expect=(tile, stage, vec))
    # A_CONVT: 16-byte form with rows of 8 pixels; the 4-byte form through rows of 7 (wide tile) / Ci = 3 pre-scaled (narrow)
    if vec:
        return wgrad(name, 3, 2, 8, 4, N, 1, force_bk=0 if stage == 64 else 16, expect=(tile, stage, vec))
    if tile == 64:
        return wgrad(name, 3, 2, 7, 4, N, 1, force_bk=0 if stage == 64 else 16, expect=(tile, stage, vec))
    return wgrad(name, 3, 2, 8, 3, N, 1, prescale=1, force_bk=0 if stage == 64 else 16, expect=(tile, stage, vec))


# which case pins which instantiation: (amode, bmode, tile, stage, vec) -> the name of the case written for it
INSTANTIATIONS = {}


def _build_pins():
    for form in ALL_FORMS:
        c = _add("pins/" + PAIR_NAME[form[:2]], _pin_case(*form))
        INSTANTIATIONS[form] = c.name


_build_plain()
_build_conv()
_build_dgrad()
_build_wgrad()
_build_epilogue()
_build_slabs()
_build_pins()
EXACT_CASES = [c for cs in GROUPS.values() for c in cs]
BY_NAME = {c.name: c for c in EXACT_CASES}
assert len(BY_NAME) == len(EXACT_CASES), "case names must be unique"


# ---- real-valued cases: one per mode pair, K <= 640, against the float32 accumulation bound --------------------------------------
def real_cases():
    all_terms = EPILOGUE_TERMS
    return [
        plain("real-row-row", A_ROW, B_ROW, 65, 100, 640, exact=False, terms=all_terms),
        plain("real-row-row-split", A_ROW, B_ROW, 65, 100, 640, exact=False, terms=all_terms, max_split=4, ldc=None, split=(4, 192)),
        plain("real-row-colt", A_ROW, B_COLT, 129, 32, 600, exact=False, terms=("bias",), max_split=2, ldc=None, split=(2, 320)),
        plain("real-col-row", A_COL, B_ROW, 68, 33, 200, exact=False, terms=("accumulate",)),
        conv("real-conv-row", 2, 5, 7, 64, 40, exact=False, terms=("bias", "alpha", "resid")),
        conv("real-conv-row-s2", 2, 5, 7, 20, 32, 3, 2, 1, exact=False, terms=("bias", "relu")),
        dgrad("real-conv-flip", 2, 5, 7, 64, 32, 2, exact=False, terms=("act",), max_split=4, ldc=None, split=(3, 192)),
        wgrad("real-convt-row", 7, 6, 9, 32, 64, 1, exact=False, max_split=128, ldc=None, split=(2, 192)),
        wgrad("real-convt-row-a2", 5, 3, 8, 4, 32, 0, exact=False, n2=2, terms=("accumulate",)),
    ]


def error_bound(c, splitk):
    """worst case of a float32 accumulation of K products, splitk slab sums and the epilogue's few roundings"""
    return (c.K + splitk + 8) * 2.0 ** -24 * magnitude(c)
