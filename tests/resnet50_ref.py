"""One-op float64 references of the VGGFace2 ResNet-50 forward (csrc/resnet50.hip), the tolerances an op is judged by in the
three types (bf16, f16, split precision f16x2), and the mutants that show the tolerances discriminate.  TEST INFRASTRUCTURE:
torch on the CPU, no GPU, nothing of the product.  Restated from oracle/vgg_resnet50.py and from what add_conv / finalize pack.

The network is 55 ops in execution order (OPS): the stem conv1/7x7_s2 (which also makes the pixels), max_pool, 52 convolutions
(per unit 1x1_reduce, 3x3, on a stage's first unit 1x1_proj, then 1x1_increase) and avg_pool.  An op is judged alone: the
reference of op i is applied to the tensors the device really left for its input (OPS[i].src) and residual (OPS[i].res), read
back through alink_debug_resnet50_embed_prefix (the stand-in's own in tests/test_resnet50_ref_host.py) and widened exactly —
16-bit to float64, pairs as (hi + lo) 2^-e — so no error is carried between layers or hidden by a later pool.

  stem pixels  (px - mean) in float32 with the RGB -> BGR flip, rounded to T; split precision: the f16 pair of v * 64, / 64.
               Padding TensorFlow 'same': total (Ho - 1) 2 + 7 - H, before = total / 2
  weights      a = gamma / sqrt(var + eps) in double, eps the float32 1e-3f widened; 16-bit: a w rounded through float32 to T
               (Round16::ViaFloat32); split precision: a w in double (the device keeps its f16 pair: 2^-22, inside the bound);
               bias float32(beta - mu a)
  convolution  act(conv(A, W) + bias [+ R]): ReLU after reduce and 3x3, none on proj, ReLU of the sum on increase, the stride
               on the first 1x1
  pools        max_pool2d(A, 3, 2) 'valid'; the mean over the 7 x 7 map

Tensors are (n, C, H, W) float64 here; nhwc() / nchw() convert from and to the device's (n, H, W, C).

Tolerances (|got - ref| <= tol, per output):
  16-bit conv / stem   REL[T] |ref| + 2e-3 max(1, s), s = sqrt(K) rms(A) rms(W_T) per image, K = k k Cin (147 for the stem): the
                       bound of tests/vgg16_ref.py (tests/test_gpu_conv.py's, whose operands are drawn for s = 1; a convolution
                       is linear in its input, so every error term of the kernel scales with s).  REL = 2^-8 (bf16), 2^-10
                       (f16): half an ulp of T at the reference and more.  The residual is a 16-bit value added exactly in
                       float32: no term of its own
  16-bit max-pool      exact: a maximum of 16-bit values is one of them
  16-bit average pool  a sequential float32 sum of 49 exact values (48 roundings, each <= 2^-24 of a partial sum <= sum |A|), the
                       rounding of 1 / 49 and one multiply: <= 50 2^-24 mean |A|
  f16x2 conv / stem    4e-6 mag, mag the same reference on |A|, |W|, |bias|, |R|: what test_split_precision_conv_matches_f64
                       asserts for these kernels (2^-22 per stored operand, the dropped lo x lo term, float32 accumulation)
  f16x2 max-pool       in stored units, m the exact maximum of hi + lo: one float32 rounding of hi + lo (2^-24 |m|, taken as
                       2^-23) and the re-split into a pair (2^-22 |m|, or half the f16 subnormal spacing 2^-25 where lo is
                       subnormal): 2^-23 |m| + max(2^-22 |m|, 2^-25)
  f16x2 average pool   the 16-bit bound on hi + lo, times the scale 2^-e
"""
import collections

import numpy as np
import torch
import torch.nn.functional as F

UNITS = (3, 4, 6, 3)
MID = (64, 128, 256, 512)
MEAN_BGR = (91.4953, 103.8827, 131.0912)
EPS32 = float(np.float32(1e-3))                 # r->eps: the float32 1e-3f, widened
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
TYPES = ("bf16", "f16", "f16x2")
REL = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}
FLOOR = 2e-3
X2_REL = 4e-6

# kind: stem | maxpool | conv | avgpool; role (conv): reduce | 3x3 | proj | increase; src / res: the ops whose outputs are this
# op's input / residual (None: the pixels / no residual); unit_in: the op whose output is the unit's input
Op = collections.namedtuple("Op", "kind name role k stride cin cout src res relu post_relu unit_in")


def _ops():
    ops = [Op("stem", "conv1/7x7_s2", None, 7, 2, 3, 64, None, None, True, False, None),
           Op("maxpool", "max_pool", None, 3, 2, 64, 64, 0, None, False, False, None)]
    x, cin = 1, 64
    for s in range(4):
        mid, out = MID[s], 4 * MID[s]
        for u in range(1, UNITS[s] + 1):
            p = "conv%d_%d_" % (s + 2, u)
            st = 2 if (u == 1 and s > 0) else 1
            i = len(ops)
            ops.append(Op("conv", p + "1x1_reduce", "reduce", 1, st, cin, mid, x, None, True, False, x))
            ops.append(Op("conv", p + "3x3", "3x3", 3, 1, mid, mid, i, None, True, False, x))
            res = x
            if u == 1:
                ops.append(Op("conv", p + "1x1_proj", "proj", 1, st, cin, out, x, None, False, False, x))
                res = len(ops) - 1
            ops.append(Op("conv", p + "1x1_increase", "increase", 1, 1, mid, out, i + 1, res, False, True, x))
            x, cin = len(ops) - 1, out
    ops.append(Op("avgpool", "avg_pool", None, 7, 1, 2048, 2048, x, None, False, False, None))
    return ops


OPS = _ops()
assert len(OPS) == 55 and sum(o.kind == "conv" for o in OPS) == 52


def tensor_shapes():
    t = {}
    for o in OPS:
        if o.kind in ("stem", "conv"):
            t[o.name + "/kernel"] = (o.k, o.k, o.cin, o.cout)
            for s in ("gamma", "beta", "moving_mean", "moving_variance"):
                t[o.name + "/bn/" + s] = (o.cout,)
    return t


def draw_params(seed, beta_std=0.5):
    """He-normal kernels and BN statistics such that, on images of unit scale, activations stay of order one through all
    sixteen units: a convolution of a ReLU'd unit-scale map with He weights has variance ~ 2 E[x^2], the moving variance is
    drawn around that (1 .. 3), gamma around 1 (0.2 .. 0.5 on 1x1_increase, as trained residual nets have their last BN small).
    Betas and moving means of standard deviation beta_std: a bias read from the wrong channel then moves an output by ~ 0.7
    beta_std, far beyond any tolerance here (the product's synthetic_params draws 0.1 against activations of 100 on raw
    pixels)."""
    rng = np.random.default_rng(seed)
    p = {}
    for name, shape in tensor_shapes().items():
        if name.endswith("/kernel"):
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))
        elif name.endswith("gamma"):
            v = rng.uniform(0.2, 0.5, shape) if "increase" in name else rng.uniform(0.7, 1.3, shape)
        elif name.endswith("beta"):
            v = rng.standard_normal(shape) * beta_std
        elif name.endswith("moving_mean"):
            v = rng.standard_normal(shape) * beta_std
        else:
            v = rng.uniform(1.0, 3.0, shape)
        p[name] = np.ascontiguousarray(v, dtype=np.float32)
    return p


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def round_to(x32, dt):
    """float32 -> T -> float64 (dt None or 'f16x2': the float32 value itself)"""
    assert x32.dtype == torch.float32
    return (x32.to(TORCH_DT[dt]) if dt in TORCH_DT else x32).double()


# ---- f16 pairs ----------------------------------------------------------------------------------------------------------------
def split_pair(v32):
    """float32 -> (hi, lo) float16: hi = RN16(v), lo = RN16(v - hi), the subtraction in float32 (exact) as the kernels do it"""
    hi = v32.to(torch.float16)
    return hi, (v32 - hi.float()).to(torch.float16)


def scale_exp(maxabs):
    """net_host.h: the exponent e with maxabs 2^e in [1024, 2048)"""
    return 10 - int(np.floor(np.log2(maxabs))) if maxabs > 0 and np.isfinite(maxabs) else 0


def widen_pairs(raw, C):
    """the device's (n, H, W, 2 C) float16, every 64-channel chunk [hi 64 | lo 64] -> (hi, lo) as (n, H, W, C) float64"""
    n, H, W, C2 = raw.shape
    assert C2 == 2 * C and C % 64 == 0 and raw.dtype == torch.float16
    t = raw.reshape(n, H, W, C // 64, 2, 64).double()
    return t[..., 0, :].reshape(n, H, W, C), t[..., 1, :].reshape(n, H, W, C)


# ---- operands -----------------------------------------------------------------------------------------------------------------
def stem_pad(H, W):
    """(left, right, top, bottom) of TensorFlow's 'same' for the 7x7 stride-2 stem"""
    th = max((-(-H // 2) - 1) * 2 + 7 - H, 0)
    tw = max((-(-W // 2) - 1) * 2 + 7 - W, 0)
    return (tw // 2, tw - tw // 2, th // 2, th - th // 2)


def stem_pixels(x, dt, preprocessed, flip=True, means_bgr=True):
    """(n, H, W, 3) float32 pixels -> (n, 3, H, W) float64: what the stem kernels' loader parks in LDS.  flip / means_bgr False
    are two of the stem's mutants (channels left in RGB order; the means indexed by the source channel)."""
    x = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32)
    if not preprocessed:
        sub = torch.tensor(MEAN_BGR, dtype=torch.float32)
        x = (x.flip(-1) if flip else x) - (sub if means_bgr else sub.flip(0))           # float32
    if dt == "f16x2":
        hi, lo = split_pair(x * 64.0)
        return nchw((hi.double() + lo.double()) / 64.0)
    return nchw(round_to(x, dt))


def fold(params, name, eps=EPS32):
    """(a, b) in double: a = gamma / sqrt(var + eps), b = beta - mu a"""
    g, be, mu, var = (torch.from_numpy(params[name + "/bn/" + s]).double() for s in ("gamma", "beta", "moving_mean", "moving_variance"))
    a = g / torch.sqrt(var + eps)
    return a, be - mu * a


def weights_t(params, name, dt, eps=EPS32):
    """(Cout, Cin, k, k) float64 folded weights as the type holds them, and the bias float32(b) widened.  dt None: nothing is
    rounded (weights and bias in double)"""
    a, b = fold(params, name, eps)
    w = torch.from_numpy(params[name + "/kernel"]).double().permute(3, 2, 0, 1).contiguous() * a[:, None, None, None]
    if dt in TORCH_DT:
        w = round_to(w.float(), dt)
    return w, (b if dt is None else b.float().double())


# ---- the references -------------------------------------------------------------------------------------------------------------
def conv_pre(op, A, Wt, bias, R=None, pad=None):
    """the sums before any ReLU: conv(A, W) + bias [+ R]"""
    if op.kind == "stem":
        A = F.pad(A, stem_pad(A.shape[2], A.shape[3]) if pad is None else pad)
        y = F.conv2d(A, Wt, bias, stride=2)
    else:
        y = F.conv2d(A, Wt, bias, stride=op.stride, padding=op.k // 2)
    return y if R is None else y + R


def conv_ref(op, A, Wt, bias, R=None, pad=None):
    y = conv_pre(op, A, Wt, bias, R, pad)
    return F.relu(y) if (op.relu or op.post_relu) else y


def maxpool_ref(A):
    return F.max_pool2d(A, 3, 2)


def avgpool_ref(A):
    assert A.shape[2:] == (7, 7)
    return A.mean(dim=(2, 3), keepdim=True)


def op_ref(params, dt, i, A, R=None, eps=EPS32):
    """reference of op i on A (the widened output of OPS[i].src; for op 0 stem_pixels(...)) and R (of OPS[i].res).
    Returns (ref, Wt, bias): Wt, bias None for a pool"""
    op = OPS[i]
    if op.kind == "maxpool":
        return maxpool_ref(A), None, None
    if op.kind == "avgpool":
        return avgpool_ref(A), None, None
    Wt, bias = weights_t(params, op.name, dt, eps)
    return conv_ref(op, A, Wt, bias, R), Wt, bias


# ---- tolerances ---------------------------------------------------------------------------------------------------------------
def scale(A, Wt):
    """s = sqrt(K) rms(A) rms(W_T) per image, (n, 1, 1, 1)"""
    K = Wt[0].numel()
    return np.sqrt(K) * A.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt() * Wt.pow(2).mean().sqrt()


def magnitude(op, A, Wt, bias, R=None):
    """the reference on |A|, |W|, |bias|, |R|: the per-output sum of |products|"""
    return conv_pre(op, A.abs(), Wt.abs(), bias.abs(), None if R is None else R.abs())


def conv_tolerance(op, dt, ref, A, Wt, bias, R=None):
    if dt == "f16x2":
        return X2_REL * magnitude(op, A, Wt, bias, R)
    return REL[dt] * ref.abs() + FLOOR * scale(A, Wt).clamp(min=1.0)


def avgpool_tolerance(A):
    """in the units of A (split precision: stored units of hi + lo, or true units — the bound is linear)"""
    return 50 * 2.0 ** -24 * A.abs().mean(dim=(2, 3), keepdim=True)


def maxpool_x2_tolerance(m):
    """m: the exact maximum of hi + lo in stored units"""
    return 2.0 ** -23 * m.abs() + torch.clamp(2.0 ** -22 * m.abs(), min=2.0 ** -25)


def worst(got, ref, tol):
    """largest err / tol (0 / 0 counts as 0); for finite operands"""
    err = (got - ref).abs()
    return float(torch.where(err > 0, err / tol, torch.zeros_like(err)).max())


# ---- the float32 stand-in for the device -------------------------------------------------------------------------------------
def store(v32, dt):
    """a float32 result as the type stores it, widened: (value float64, e).  Split precision: the pair of v 2^e, e from the
    tensor's maximum as calibration would choose it"""
    if dt != "f16x2":
        return round_to(v32, dt), 0
    e = scale_exp(float(v32.abs().max()))
    hi, lo = split_pair(v32 * 2.0 ** e)
    return (hi.double() + lo.double()) * 2.0 ** -e, e


def conv_standin(op, A, Wt, bias, R, dt):
    """torch's float32 convolution of the same operands, the residual added in float32, stored in T or as a pair"""
    y = conv_pre(op, A.float(), Wt.float(), bias.float(), None if R is None else R.float())
    return store(F.relu(y) if (op.relu or op.post_relu) else y, dt)[0]


def avgpool_standin(A):
    """a sequential float32 sum of the 49 positions in the kernel's order, times float32(1 / 49)"""
    a = nhwc(A).float().reshape(A.shape[0], 49, A.shape[1])
    s = torch.zeros(A.shape[0], A.shape[1], dtype=torch.float32)
    for pos in range(49):
        s = s + a[:, pos]
    return (s * (torch.tensor(1.0, dtype=torch.float32) / 49.0)).double()[:, :, None, None]


# ---- mutants: references that are wrong the way a kernel or the plumbing could be ---------------------------------------------------
def _swap_adjacent(t):
    return t[:, torch.arange(t.shape[1]) ^ 1]


def _odd_positions(op, A, Wt, b, R):
    """a stride-2 1x1 that samples positions 1, 3, .. instead of 0, 2, .. (zero beyond the map)"""
    return conv_ref(op, F.pad(A[:, :, 1:, 1:], (0, 1, 0, 1)), Wt, b, R)


def resid_from_unit_input(op, A, Wt, b, R, X):
    """the residual of a first unit read from the unit's input buffer X instead of the projection's: the kernel sees flat
    [pixel][Cout] memory, so the first n Ho Wo Cout values of X in the device's order"""
    fake = nchw(nhwc(X).flatten()[:R.numel()].reshape(nhwc(R).shape))
    return conv_ref(op, A, Wt, b, fake)


def resid_from_unit_input_applies(op, R, X):
    return op.role == "increase" and op.res != op.unit_in and X.numel() >= R.numel()


# name -> (applies(op), mutant(op, A, Wt, bias, R)); R is None where the op has no residual
CONV_MUTANTS = {
    "bias rolled by one channel": (lambda op: True, lambda op, A, Wt, b, R: conv_ref(op, A, Wt, b.roll(1), R)),
    "adjacent output channels swapped": (lambda op: True, lambda op, A, Wt, b, R: _swap_adjacent(conv_ref(op, A, Wt, b, R))),
    "3x3 taps transposed": (lambda op: op.k > 1, lambda op, A, Wt, b, R: conv_ref(op, A, Wt.transpose(2, 3).contiguous(), b, R)),
    "ReLU dropped": (lambda op: op.relu, lambda op, A, Wt, b, R: conv_pre(op, A, Wt, b, R)),
    "post_relu dropped on increase": (lambda op: op.post_relu, lambda op, A, Wt, b, R: conv_pre(op, A, Wt, b, R)),
    "residual dropped": (lambda op: op.res is not None, lambda op, A, Wt, b, R: conv_ref(op, A, Wt, b, None)),
    "stride-2 1x1 sampling odd positions": (lambda op: op.kind == "conv" and op.stride == 2, _odd_positions),
}


def stem_pad_swapped(H, W):
    l, r, t, b = stem_pad(H, W)
    return (r, l, b, t)


def maxpool_late(A):
    """the windows start one pixel late (-inf beyond the map)"""
    return F.max_pool2d(F.pad(A[:, :, 1:, 1:], (0, 1, 0, 1), value=float("-inf")), 3, 2)


def avgpool_by_64(A):
    return A.sum(dim=(2, 3), keepdim=True) / 64.0


# ---- which kernel and form serve a convolution: direct_variant_tiles, linear_variant_x2 and served_form, restated --------------------
IGEMM, T14C256, T28C256, T28C128, T56C128, T56C64, T112C64, P14, P28 = 0, 1, 2, 3, 4, 5, 6, 7, 8
L14, L28, L56, L7, L112 = 11, 12, 13, 14, 15
LINEAR = (L14, L28, L56, L7, L112)
SELF, LAT3, LATG = 0, 1, 2


def expected_kernel(op, H, W, dt, linear_ok=True):
    """the ConvKernel finalize chooses for a convolution whose INPUT map is H x W (default switches: linear mode 31, pair on).
    Every 3x3 of this network has stride 1, pad 1 and Cin = Cout a multiple of 64."""
    if op.k != 3:
        return IGEMM
    C = op.cout
    if linear_ok and H == W:                                  # linear_variant (+ Linear112 in split precision)
        if W == 14 and C % 128 == 0:
            return L14
        if W == 28 and C % 128 == 0:
            return L28
        if W == 56:
            return L56
        if W == 7 and C % 128 == 0:
            return L7
        if W == 112 and dt == "f16x2":
            return L112
    if dt == "f16x2" or W > 112:                               # the row-aligned tile kernels have no split-precision form
        return IGEMM
    tr, pitch = (W + 15) // 16, (W + 2 + 15) // 16 * 16
    if tr == 1 and pitch == 16 and W >= 12 and C % 128 == 0:
        return P14                                            # S1: 69 KB at every Cin (single input buffer)
    if tr == 2 and pitch == 32 and C % 128 == 0:
        return P28                                            # S3: 73 KB
    if tr == 4 and pitch == 64 and C % 128 == 0:
        return T56C128
    if tr == 4 and pitch == 64 and op.cin == 64:               # D5 fits only a single input buffer (Cin 64)
        return T56C64
    return IGEMM


def expected_form(op, kernel, n, Hin, Win, Ho, Wo, latency_pixels=1600):
    """served_form: conv3x3_lat_applies for the linear-tile kernels, conv_gemm_lat_applies for the implicit GEMM's 1x1 layers
    (the byte-offset limits of both hold at every size here)"""
    if latency_pixels <= 0:
        return SELF
    if kernel in LINEAR:
        pix = n * Hin * Win
        ok = op.cin >= 128 and pix <= latency_pixels and (pix + 31) // 32 * (op.cout // 32) <= 448
        return LAT3 if ok else SELF
    if kernel == IGEMM and op.k == 1:
        M = n * Ho * Wo
        ok = op.cin // 64 in (1, 2, 4, 8) and M <= 784 and (M + 15) // 16 * (op.cout // 16) <= 512
        return LATG if ok else SELF
    return SELF


def shapes(H, W):
    """[(Hin, Win, Hout, Wout)] per op for an H x W image"""
    out, dims = [], {}
    for i, op in enumerate(OPS):
        if op.kind == "stem":
            hi, wi, ho, wo = H, W, -(-H // 2), -(-W // 2)
        else:
            hi, wi = dims[op.src]
            if op.kind == "maxpool":
                ho, wo = (hi - 3) // 2 + 1, (wi - 3) // 2 + 1
            elif op.kind == "avgpool":
                ho, wo = 1, 1
            else:
                ho, wo = (hi - 1) // op.stride + 1, (wi - 1) // op.stride + 1
        dims[i] = (ho, wo)
        out.append((hi, wi, ho, wo))
    return out


def expected_table(H, W, n, dt, latency_pixels=1600, linear_ok=True):
    """[(kernel, form)] per op for chunks of n images: (-1, 0) for the stem and the pools"""
    rows = []
    for op, (hi, wi, ho, wo) in zip(OPS, shapes(H, W)):
        if op.kind != "conv":
            rows.append((-1, 0))
            continue
        k = expected_kernel(op, hi, wi, dt, linear_ok)
        rows.append((k, expected_form(op, k, n, hi, wi, ho, wo, latency_pixels)))
    return rows
