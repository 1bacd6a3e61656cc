"""One-op float64 references of the VGG-16 forward (csrc/vgg16.hip), the tolerance a 16-bit layer is judged by, and the
mutants that show the tolerance discriminates.  TEST INFRASTRUCTURE: torch on the CPU, no GPU, nothing of the product.

The network is 18 ops in execution order (OPS): conv1_1 (the stem kernel, which also makes the pixels), twelve convolutions
and five pools.  A layer is judged alone: the reference of op i is applied to the 16-bit tensor op i - 1 really left (the
device's own, read back through alink_debug_vgg16_embed_prefix; the stand-in's in tests/test_vgg16_ref_host.py), widened
exactly, so no error is carried from layer to layer and none can hide behind a later max-pool.

  stem pixels  (px - sub) * mul in float32 with the RGB -> BGR flip (slot 2 - c takes channel c and mean 2 - c), rounded to T
  convolution  ReLU(conv(A, W_T) + bias): W_T the float32 Keras kernel rounded to T (the packers' Round16::ViaFloat32), the
               bias float32, A the 16-bit input; float64 sums
  pool         max_pool2d(A, 2, 2), floor mode; torch's keeps NaN, as maxpool2_kernel's max_keep_nan does

Tensors are (n, C, H, W) float64 here; nhwc() / nchw() convert from and to the device's (n, H, W, C).

Tolerance: the bound tests/test_gpu_conv.py asserts for the 16-bit kernels, |got - ref| <= rel |ref| + 2e-3 with rel = 2^-8
(bf16) / 2^-10 (f16), holds there for operands drawn so that an output has unit scale: s = sqrt(K) rms(A) rms(W_T) = 1, K = 9 Cin.
A convolution is linear in its input, so every error term of the kernel (the products' f32 summation, the rounding of the stored
value) scales with s, and the floor does: 2e-3 max(1, s), s taken per image.  rel |ref| is half an ulp of T at the reference
and more: bf16 keeps 8 bits (half an ulp <= 2^-9 |ref|), f16 11 (2^-12)."""
import numpy as np
import torch
import torch.nn.functional as F

BLOCKS = (2, 2, 3, 3, 3)
MEAN_BGR = (93.5940, 104.7624, 129.1863)
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
REL = {"bf16": 2.0 ** -8, "f16": 2.0 ** -10}
FLOOR = 2e-3


def _ops():
    out = []
    for b in range(5):
        for l in range(BLOCKS[b]):
            out.append(("stem" if (b, l) == (0, 0) else "conv", "conv%d_%d" % (b + 1, l + 1)))
        out.append(("pool", "pool%d" % (b + 1)))
    return out


OPS = _ops()                     # [(kind, name)] in execution order
assert len(OPS) == 18


def draw_params(seed, bias_std=0.5):
    """the kernels of a_link_amd.vgg16.synthetic_params (He), biases of standard deviation bias_std: on activations of unit
    scale a bias read from the wrong channel then moves an output by ~0.7, far beyond any 16-bit tolerance (with the
    product's own 0.05 on raw pixels, activations ~100, it moves next to nothing)"""
    from a_link_amd import vgg16 as V
    p = V.synthetic_params(seed)
    rng = np.random.default_rng(seed + 1000)
    for name in p:
        if name.endswith("/bias"):
            p[name] = np.ascontiguousarray(rng.standard_normal(p[name].shape) * bias_std, dtype=np.float32)
    return p


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def round_to(x32, dt):
    """float32 -> T -> float64 (dt None: no rounding, the float32 value itself)"""
    assert x32.dtype == torch.float32
    return (x32 if dt is None else x32.to(TORCH_DT[dt])).double()


def stem_pixels(x, dt, preprocessed, flip=True, means_bgr=True):
    """(n, H, W, 3) float32 pixels -> (n, 3, H, W) float64: what stem_kernel's loader parks in LDS.  flip / means_bgr False
    are the stem's two mutants (channels left in RGB order; the means indexed by the source channel)."""
    x = torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32)
    if not preprocessed:
        sub = torch.tensor(MEAN_BGR, dtype=torch.float32)
        x = (x.flip(-1) if flip else x) - (sub if means_bgr else sub.flip(0))           # float32; VGG-16's mul is 1
    return nchw(round_to(x, dt))


def weights_t(params, name, dt):
    """(Cout, Cin, 3, 3) float64: the Keras kernel (3, 3, Cin, Cout) rounded to T from float32"""
    return round_to(torch.from_numpy(params[name + "/kernel"]).permute(3, 2, 0, 1).contiguous(), dt)


def bias_of(params, name):
    return torch.from_numpy(params[name + "/bias"]).double()


def conv_pre(A, Wt, bias):
    """the convolution's sums before the ReLU"""
    return F.conv2d(A, Wt, bias, padding=1)


def conv_ref(A, Wt, bias):
    return F.relu(conv_pre(A, Wt, bias))


def pool_ref(A):
    return F.max_pool2d(A, 2, 2)


def conv_standin(A, Wt, bias, dt):
    """a stand-in for the device: torch's float32 convolution of the same operands, stored in T"""
    return round_to(F.relu(F.conv2d(A.float(), Wt.float(), bias.float(), padding=1)), dt)


def op_ref(params, dt, i, A):
    """reference of op i on A, the (widened) output of op i - 1 — for op 0, stem_pixels(...).  Returns (ref, Wt): Wt None for a pool"""
    kind, name = OPS[i]
    if kind == "pool":
        return pool_ref(A), None
    Wt = weights_t(params, name, dt)
    return conv_ref(A, Wt, bias_of(params, name)), Wt


def scale(A, Wt):
    """s = sqrt(K) rms(A) rms(W_T) per image, (n, 1, 1, 1)"""
    K = Wt[0].numel()
    return np.sqrt(K) * A.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt() * Wt.pow(2).mean().sqrt()


def tolerance(ref, A, Wt, dt):
    return REL[dt] * ref.abs() + FLOOR * scale(A, Wt).clamp(min=1.0)


def worst(got, ref, tol):
    """largest err / tol; NaN-safe only for finite operands"""
    return float(((got - ref).abs() / tol).max())


# ---- mutants: references that are subtly wrong, each the way a kernel could be ------------------------------------------------
def _swap_adjacent(t):
    idx = torch.arange(t.shape[1]) ^ 1
    return t[:, idx]


def _valid_only(A, Wt, bias):
    """zero padding replaced by a valid convolution: the interior is the same sums, the border ring is never written (0)"""
    out = torch.zeros(A.shape[0], Wt.shape[0], A.shape[2], A.shape[3], dtype=A.dtype)
    out[:, :, 1:-1, 1:-1] = F.relu(F.conv2d(A, Wt, bias))
    return out


CONV_MUTANTS = {
    "bias rolled by one channel": lambda A, Wt, b: conv_ref(A, Wt, b.roll(1)),
    "taps transposed": lambda A, Wt, b: conv_ref(A, Wt.transpose(2, 3).contiguous(), b),
    "adjacent output channels swapped": lambda A, Wt, b: _swap_adjacent(conv_ref(A, Wt, b)),
    "ReLU dropped": lambda A, Wt, b: conv_pre(A, Wt, b),
    "valid convolution (border)": _valid_only,
}


def pool_shifted(A):
    """the pool's mutant on an odd map: the windows start at the odd row / column, so the LAST row / column is kept and the
    first dropped (the floor rule drops the last)"""
    return F.max_pool2d(A[:, :, A.shape[2] % 2:, A.shape[3] % 2:], 2, 2)
