"""GPU: the two input-gradient passes (VGGFace2 ResNet-50: csrc/resnet50.hip from alink_resnet50_input_grad on +
csrc/resnet50_bwd.hip; IR backbone: alink_embed_input_grad in csrc/backbone.hip + csrc/backward.hip) against a float64
reference that shares the kernels' masks.

tests/test_gpu_resnet50_grad.py and tests/test_gpu_grad.py compare with plain autograd; there the yardstick is the noise of
ReLU masks that flip when the forward's activations are stored in 16 bits (rel 0.1 .. 0.3), and nothing smaller than a
dropped branch is seen.  Here the reference is LINEAR BY CONSTRUCTION: the oracle's forward restated with folded weights
(rounded to the mode's type the way finalize rounds them: float64 product -> float32 -> 16 bit), every ReLU / PReLU replaced
by a multiplication with a mask given from outside, the max-pool seeing the stored stem map's values (torch's CPU max-pool
gives a tie to the first maximum in row-major order: the rule r50_maxpool_bwd_kernel states), and the IR backbone's L2
normalisation linearised at the embedding and row norm the GPU forward produced.  The masks are read from the activation
cache the backward itself reads, in the caller's workspace (alink_debug_*_grad_cache_info, include/alink_hip_debug.h).  What
is left between the GPU and that reference is the rounding of the stored 16-bit gradient tensors and the f32 summation order.

The bound is measured on the reference alone: E_mask = distance (per image: rel and 1 - cos) between the reference and
the same reference with every STORED GRADIENT TENSOR rounded to the mode's type (a backward hook wherever the GPU pass
stores one: after every backward convolution — the masks and the zero-insert / scatter that follow a store are exact on
rounded values — and after the pool backward), under the call's own power-of-two gradient scale where the pass has one
(ResNet-50).  The GPU must stay within 2 x E_mask in rel and 4 x E_mask in 1 - cos; the factor covers another realisation of
the same roundings (f32 accumulation order, a store one operation earlier or later than the hook) and is not tuned on a GPU
result.  That the bound discriminates is checked on the CPU in the same test: every mutant of the REFERENCE (never of the
GPU side) must move it by more than 2 x the bound, for every image.

IR backbone weights: the synthetic draw sets every PReLU slope to 0.25, under which a slope read from the wrong channel
changes nothing; the tests redraw the slopes per channel (uniform 0.05 .. 0.45) before the BatchNorm statistics are set.

Measured on MI355X, rel per image (min - max over the case's images; 1 - cos and every mutant: DESIGN.md §9, "Accuracy against a
reference sharing the kernels' masks"):
  ResNet-50 bf16  224 x 224 n=3   GPU 8.77e-3 - 9.02e-3   E_mask 8.59e-3 - 9.02e-3   (bound 1.72e-2 - 1.80e-2)
            f16   224 x 224 n=3   GPU 1.09e-3 - 1.12e-3   E_mask 1.08e-3 - 1.13e-3
            bf16  201 x 215 n=2   GPU 8.45e-3 - 8.66e-3   E_mask 8.43e-3 - 8.78e-3
            f16   201 x 215 n=2   GPU 1.04e-3 - 1.08e-3   E_mask 1.06e-3 - 1.09e-3   (raw and preprocessed alike)
            bf16  224 x 199 n=2   GPU 8.82e-3 - 8.93e-3   E_mask 8.76e-3 - 8.95e-3
            f16   224 x 199 n=2   GPU 1.10e-3 - 1.13e-3   E_mask 1.11e-3 - 1.13e-3
            bf16  224 x 224 n=34  GPU 8.31e-3 - 9.11e-3   E_mask 8.20e-3 - 9.13e-3
  IR (2,2,2,2)  bf16 n=4          GPU 6.79e-3 - 6.91e-3   E_mask 6.83e-3 - 6.97e-3
                f16 normalized    GPU 8.04e-4 - 8.27e-4   E_mask 8.12e-4 - 8.33e-4   (NCHW)
                bf16 n=34         GPU 6.71e-3 - 7.03e-3   E_mask 6.70e-3 - 6.98e-3
  IR (3,4,14,3) bf16 n=4          GPU 1.10e-2 - 1.16e-2   E_mask 1.11e-2 - 1.15e-2
                f16 normalized    GPU 1.20e-3 - 1.24e-3   E_mask 1.20e-3 - 1.22e-3
The GPU sits at 0.97 - 1.03 x E_mask everywhere; the nearest mutant (ResNet-50 bf16, stem ReLU mask not applied, 0.073) is
4.3 x the bound away, the last-maximum tie rule 5.1 x (bf16) / 13.6 x (f16), every other one 5.4 x and more.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

gpu_test = pytest.mark.gpu               # every test that touches the device; the reference's own check runs without one

TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
R50_UNITS = (3, 4, 6, 3)                 # the VGGFace2 ResNet-50's bottleneck units per stage
MEAN_BGR = (91.4953, 103.8827, 131.0912)
CHUNK = 4                                # images per float64 pass (the reference is independent per image)


def _threads():
    torch.set_num_threads(min(16, os.cpu_count() or 1))


def _rel_cos(g, ref):
    a, b = np.asarray(g, np.float64).reshape(len(g), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return rel, 1.0 - cos


def _r16(v, dt):
    """float64 -> float32 -> the 16-bit type -> float64: what a kernel's f32 result becomes when it is stored"""
    return v.float().to(dt).double()


def _hook(v, dt):
    if dt is not None and v.requires_grad:
        v.register_hook(lambda g: _r16(g, dt))
    return v


def _t(params, name):
    return torch.from_numpy(np.ascontiguousarray(params[name])).double()


# ---- the VGGFace2 ResNet-50 ------------------------------------------------------------------------------------------------
def r50_grad(params, x, dfeat, masks=None, wround=None, ground=None, gscale=1.0, mutate=None, record=None, preprocessed=False,
             eps=float(np.float32(1e-3))):
    """d(sum(features * dfeat)) / d(x) in float64.  x: (N, H, W, 3) raw RGB, or preprocess_input(version=2)'d (BGR, means
    subtracted) with preprocessed=True; the gradient comes in x's own channel order.
    masks None: the oracle's forward itself (oracle/vgg_resnet50.forward with BatchNorm folded), ReLUs and all; `record`
    receives the post-ReLU tensors under the cache's names.  Returns (features, gradient).
    masks: name -> stored tensor (N, C, H, W): every ReLU multiplies by (stored > 0), the pool sees masks["stem"]'s values.
    wround: folded weights rounded to this type; ground: stored gradients rounded to it, dfeat scaled by gscale on the way in
    and the result by 1 / gscale; mutate: one deliberate mistake (see R50_MUTANTS); eps: BatchNorm's, the float32 value the
    library folds with."""
    def act(pre, name):
        if masks is None:
            v = F.relu(pre)
            if record is not None:
                record[name] = v.detach().clone()
            return v
        _hook(pre, ground)               # the GPU stores d(loss)/d(pre-activation): the mask rides in the producing launch
        m = (masks[name] > 0).double()
        if mutate == ("ones", name):
            m = torch.ones_like(m)
        return pre * m

    def conv_bn(v, name, stride=1, pad=0):
        w = _t(params, name + "/kernel").permute(3, 2, 0, 1).contiguous()
        g, b, mu, var = (_t(params, name + "/bn/" + s) for s in ("gamma", "beta", "moving_mean", "moving_variance"))
        a = g / torch.sqrt(var + eps)
        wf = a[:, None, None, None] * w
        if wround is not None:
            wf = _r16(wf, wround)
        if mutate == ("noflip", name):
            wf = wf.flip(2, 3)
        return F.conv2d(v, wf, stride=stride, padding=pad) + (b - mu * a)[None, :, None, None]

    xr = torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(True)
    if preprocessed:
        v = xr
    else:   # the means are subtracted in float32 (so does the stem kernel's loader): a constant offset, exact in float64
        flipped = xr.detach().float().flip(-1)
        v = xr.flip(-1) + ((flipped - torch.tensor(MEAN_BGR, dtype=torch.float32)).double() - flipped.double())
    v = v.permute(0, 3, 1, 2)
    H, W = v.shape[2], v.shape[3]
    th = max((-(-H // 2) - 1) * 2 + 7 - H, 0)
    tw = max((-(-W // 2) - 1) * 2 + 7 - W, 0)
    top = th // 2 + (1 if mutate == ("pad_t",) else 0)
    v = F.pad(v, (tw // 2, tw - tw // 2, top, th - top))
    v = act(conv_bn(v, "conv1/7x7_s2", stride=2), "stem")
    if masks is not None:
        v = masks["stem"] + (v - v.detach())
    if mutate == ("pool_last",):    # the same windows visited from the far corner: a tie goes to the LAST maximum
        r0, c0 = (1 if v.shape[2] % 2 == 0 else 0), (1 if v.shape[3] % 2 == 0 else 0)
        v = F.max_pool2d(v.flip(2).flip(3)[:, :, r0:, c0:], 3, 2).flip(2).flip(3)
    else:
        v = F.max_pool2d(v, 3, 2)
    if record is not None:
        record["pool"] = v.detach().clone()
    for s in range(4):
        for u in range(1, R50_UNITS[s] + 1):
            p = "conv%d_%d_" % (s + 2, u)
            if u == 1 and s > 0:
                v = v[:, :, ::2, ::2]    # a stride-2 1x1 reads the even positions; its backward runs on the small map
            _hook(v, ground)             # d(unit input): 1x1_reduce's backward + the shortcut's gradient, one store
            y = act(conv_bn(v, p + "1x1_reduce"), p + "reduce")
            y = act(conv_bn(y, p + "3x3", pad=1), p + "3x3")
            y = conv_bn(y, p + "1x1_increase")
            sc = conv_bn(_hook(v.clone(), ground), p + "1x1_proj") if u == 1 else v      # the projection's backward: a store
            if mutate == ("noshortcut", p[:-1]):
                sc = sc.detach()
            v = act(y + sc, p + "out")
    f = v.mean((2, 3))
    d = torch.from_numpy(np.ascontiguousarray(dfeat)).double() * gscale
    (f * d).sum().backward()
    return f.detach().numpy(), xr.grad.numpy() / gscale


R50_MUTANTS = [("ones", "stem"), ("pool_last",), ("pad_t",), ("noflip", "conv2_2_3x3"), ("noflip", "conv3_1_3x3"),
               ("noflip", "conv4_4_3x3"), ("noflip", "conv5_3_3x3"), ("ones", "conv3_1_reduce"), ("ones", "conv5_3_3x3"),
               ("noshortcut", "conv4_4")]


def r50_gscale(dfeat):
    """r50_grad_scale_kernel: 2^e with max|dfeat| 2^e / 49 in [1, 2), from the whole call's dfeat, in float32"""
    m = np.float32(np.abs(dfeat).max()) * np.float32(1.0 / 49.0)
    if not (m > 0 and np.isfinite(m)):
        return 1.0
    return 2.0 ** -(math.frexp(float(m))[1] - 1)


# ---- the IR backbone ---------------------------------------------------------------------------------------------------------
def ir_units(params):
    return [max(u for u in range(1, 200) if "stage%d_unit%d_conv1_weight" % (s, u) in params) for s in range(1, 5)]


def ir_grad(params, x, dz, masks=None, wround=None, ground=None, mutate=None, record=None, eps=float(np.float32(2e-5))):
    """d(sum(z * dz)) / d(x) in float64 through oracle/ir_resnet.forward_raw restated with BatchNorm folded as
    csrc/backbone.hip's finalize folds it; z = the un-normalised fc1 output, x: (N, H, W, 3) RGB 0..255.  masks / wround /
    ground / mutate / record as in r50_grad; the PReLU mask is 1 where stored > 0 and the channel's slope elsewhere.  The
    stem's folded weights stay float32 in the backward (stem_bwd_kernel reads them so).  Returns (z, gradient)."""
    def bn(name, fix_gamma=False):
        g = torch.ones_like(_t(params, name + "_gamma")) if fix_gamma else _t(params, name + "_gamma")
        a = g / torch.sqrt(_t(params, name + "_moving_var") + eps)
        return a, _t(params, name + "_beta") - _t(params, name + "_moving_mean") * a

    def rw(w):
        return w if wround is None else _r16(w, wround)

    def prelu(pre, name, alpha, store):
        if masks is None:
            v = torch.where(pre > 0, pre, pre * alpha[None, :, None, None])
            if record is not None:
                record[name] = v.detach().clone()
            return v
        if store:
            _hook(pre, ground)
        a = alpha
        if mutate == ("slope0", name):
            a = torch.zeros_like(a)
        if mutate == ("next_slope", name):
            a = torch.roll(a, -1)
        return pre * torch.where(masks[name] > 0, torch.ones_like(masks[name]), a[None, :, None, None].expand_as(masks[name]))

    units = ir_units(params)
    xr = torch.from_numpy(np.ascontiguousarray(x)).double().requires_grad_(True)
    v = (xr.permute(0, 3, 1, 2) - 127.5) * 0.0078125
    a0, b0 = bn("bn0")
    w0 = a0[:, None, None, None] * _t(params, "conv0_weight")
    if wround is not None:
        w0 = w0.float().double()
    # the stem's PReLU': applied in float32 inside stem_bwd_kernel, nothing stored between it and the pixels
    v = prelu(F.conv2d(v, w0, padding=1) + b0[None, :, None, None], "stem", _t(params, "relu0_gamma"), False)
    for s in range(4):
        for u in range(units[s]):
            p = "stage%d_unit%d" % (s + 1, u + 1)
            _hook(v, ground)             # d(unit input): conv1's backward + the shortcut's gradient, one store
            (a1, b1), (a2, b2), (a3, b3) = bn(p + "_bn1"), bn(p + "_bn2"), bn(p + "_bn3")
            w1 = _t(params, p + "_conv1_weight")
            w1s = a2[:, None, None, None] * w1
            # bn1's shift reaches the output through the zero-padded convolution: a constant map (no gradient)
            shift = F.conv2d(b1[None, :, None, None].expand(1, -1, v.shape[2], v.shape[3]), w1s, padding=1) + b2[None, :, None, None]
            y = F.conv2d(v, rw(w1s * a1[None, :, None, None]), padding=1) + shift
            y = prelu(y, p + "_conv1", _t(params, p + "_relu1_gamma"), True)
            w2 = rw(a3[:, None, None, None] * _t(params, p + "_conv2_weight"))
            if u == 0 and mutate == ("odd", s):     # the stride-2 gradient placed on the odd positions of the zero map
                y = F.conv2d(y, w2, padding=1)[:, :, 1::2, 1::2]
            else:
                y = F.conv2d(y, w2, stride=2 if u == 0 else 1, padding=1)
            y = y + b3[None, :, None, None]
            if u == 0:
                asc, bsc = bn(p + "_sc")
                xs = _hook(v[:, :, ::2, ::2].clone(), ground)                            # the shortcut's backward: a store
                sc = F.conv2d(xs, rw(asc[:, None, None, None] * _t(params, p + "_conv1sc_weight"))) + bsc[None, :, None, None]
            else:
                sc = v
            if mutate == ("noshortcut", p):
                sc = sc.detach()
            v = y + sc
    _hook(v, ground)                     # the transposed FC's output
    (al, bl), (af, bf) = bn("bn1"), bn("fc1", fix_gamma=True)
    fw = _t(params, "pre_fc1_weight")
    hw = v.shape[2] * v.shape[3]
    wfc = af[:, None] * fw * al.repeat_interleave(hw)[None, :]
    bias = af * (_t(params, "pre_fc1_bias") + fw @ bl.repeat_interleave(hw)) + bf
    z = v.flatten(1) @ rw(wfc).t() + bias
    d = torch.from_numpy(np.ascontiguousarray(dz)).double()
    if ground is not None:
        d = _r16(d, ground)              # l2norm_bwd_kernel stores d(z) in the mode's type
    (z * d).sum().backward()
    return z.detach().numpy(), xr.grad.numpy()


def ir_mutants(units):
    last = "stage3_unit%d" % units[2]
    return [("slope0", "stem"), ("next_slope", "stage2_unit1_conv1"), ("next_slope", last + "_conv1"), ("odd", 0), ("odd", 2),
            ("noshortcut", "stage2_unit2"), ("noshortcut", last)]


def ir_params(units, normalized, seed=4):
    from a_link_amd import weights as W
    p = W.synthetic_ir_params(units, seed=seed, normalized=False)
    rng = np.random.default_rng(seed + 100)
    for k in p:
        if "relu" in k:
            p[k] = rng.uniform(0.05, 0.45, p[k].shape).astype(np.float32)
    if normalized:
        W.normalize_bn_statistics_(p, units)
    return p


# ---- shared machinery ------------------------------------------------------------------------------------------------------
def _chunked(fn, x, d, masks, **kw):
    out = []
    for i in range(0, len(x), CHUNK):
        m = None if masks is None else {k: v[i:i + CHUNK] for k, v in masks.items()}
        out.append(fn(x[i:i + CHUNK], d[i:i + CHUNK], masks=m, **kw)[1])
    return np.concatenate(out)


def masked_figures(fn, x, d, masks, dt, mutants, gscale=None):
    """(g_ref, E_rel, E_cos, {mutant: rel per image}) of the masked reference `fn(x, d, masks=, wround=, ground=, mutate=)`"""
    _threads()
    g_ref = _chunked(fn, x, d, masks, wround=dt)
    kw = {} if gscale is None else {"gscale": gscale}
    E_rel, E_cos = _rel_cos(_chunked(fn, x, d, masks, wround=dt, ground=dt, **kw), g_ref)
    moved = {m: _rel_cos(_chunked(fn, x, d, masks, wround=dt, mutate=m), g_ref)[0] for m in mutants}
    return g_ref, E_rel, E_cos, moved


def _cache(lib, query, handle, n, ws, dt):
    """name -> (n, C, H, W) float64 CPU copy of every tensor the backward reads from the caller's gradient workspace `ws`
    (a uint8 tensor whose first 256-byte aligned address is the workspace pointer); "norms" -> (n,) float64"""
    fn = getattr(lib, query)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                   C.c_char_p, C.c_int]
    count = fn(handle, n, -1, None, None, None, None, None, 0)
    assert count > 0, lib.alink_last_error()
    torch.cuda.synchronize()
    base = (-ws.data_ptr()) % 256
    out = {}
    for i in range(count):
        off, h, w, c, name = C.c_size_t(), C.c_int(), C.c_int(), C.c_int(), C.create_string_buffer(64)
        assert fn(handle, n, i, C.byref(off), C.byref(h), C.byref(w), C.byref(c), name, 64) == count
        key = name.value.decode()
        if key == "norms":
            out[key] = ws[base + off.value: base + off.value + 4 * n].view(torch.float32).double().cpu()
            continue
        nb = n * h.value * w.value * c.value * 2
        assert base + off.value + nb <= ws.numel(), (key, off.value, nb, ws.numel())
        t = ws[base + off.value: base + off.value + nb].view(dt).view(n, h.value, w.value, c.value)
        out[key] = t.double().cpu().permute(0, 3, 1, 2).contiguous()
    return out


def _judge(case, g_gpu, g_ref, E_rel, E_cos, moved):
    """print the case's line per image, then assert: the GPU inside 2 x E_mask (rel) / 4 x E_mask (1 - cos), every mutant of the
    reference outside 2 x the bound, for every image"""
    assert g_gpu.shape == g_ref.shape and np.isfinite(g_gpu).all()
    rel, omc = _rel_cos(g_gpu, g_ref)
    b_rel, b_cos = 2.0 * E_rel, 4.0 * E_cos
    weakest = min(moved, key=lambda m: (moved[m] / b_rel).min()) if moved else None
    for i in range(len(rel)):
        row = "%-46s img %2d  GPU rel %.3e  E_mask %.3e  bound %.3e | 1-cos %.3e  E %.3e  bound %.3e" % (
            case, i, rel[i], E_rel[i], b_rel[i], omc[i], E_cos[i], b_cos[i])
        if weakest is not None:
            row += " | smallest mutant %s %.3e" % ("/".join(str(v) for v in weakest), moved[weakest][i])
        print(row)
    for m, r in moved.items():
        print("%-46s mutant %-32s moves the reference by %s" % (case, "/".join(str(v) for v in m), np.array2string(r, precision=4)))
    assert (E_rel > 0).all() and (E_cos > 0).all()
    bad = [i for i in range(len(rel)) if not (rel[i] <= b_rel[i] and omc[i] <= b_cos[i])]
    assert not bad, "%s: images %s outside the bound: rel %s (bound %s), 1 - cos %s (bound %s)" % (case, bad, rel, b_rel, omc, b_cos)
    for m, r in moved.items():
        assert (r > 2.0 * b_rel).all(), "%s: mutant %s moves the reference by %s, not outside 2 x the bound %s" % (case, m, r, b_rel)


# ---- ResNet-50 cases ---------------------------------------------------------------------------------------------------------
_R50_PARAMS = {}


def _r50_params():
    from a_link_amd import resnet50 as R
    if not _R50_PARAMS:
        _R50_PARAMS.update(R.synthetic_params(1))
    return _R50_PARAMS


def _r50_inputs(size, n, preprocessed, seed=0):
    from oracle import vgg_resnet50 as O
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (n,) + size + (3,)).astype(np.float32)
    dfeat = rng.standard_normal((n, 2048)).astype(np.float32)
    return (O.preprocess_input_v2(x) if preprocessed else x), dfeat


def _r50_gpu(gpu, dtype, size, x, dfeat, preprocessed, want_cache=True):
    from a_link_amd.resnet50 import VGGResNet50
    n = len(x)
    net = VGGResNet50(image_size=size, weights=_r50_params(), dtype=dtype, max_batch=n, enable_grad=True)
    xd, dfd = torch.from_numpy(x).cuda(), torch.from_numpy(dfeat).cuda()
    feat = net.embed_with_cache(xd, preprocessed=preprocessed)
    assert torch.equal(feat, net.embed_device(xd, preprocessed=preprocessed)), "the cached forward is not the plain forward bit for bit"
    g = net.input_gradient(dfd)
    cache = _cache(gpu.load(), "alink_debug_resnet50_grad_cache_info", net.h, n, net.ws.tensor("grad"), TORCH_DT[dtype]) if want_cache else None
    return feat.cpu(), g.cpu().numpy(), cache


def _r50_case(gpu, dtype, size, n, preprocessed=False, mutants=R50_MUTANTS):
    x, dfeat = _r50_inputs(size, n, preprocessed)
    _, g, cache = _r50_gpu(gpu, dtype, size, x, dfeat, preprocessed)
    # the cache is what it says: 3 + 3 x 16 tensors, post-ReLU, the pooled map the max-pool of the stem map (exact: a maximum)
    assert len(cache) == 2 + 3 * sum(R50_UNITS) and all(float(v.min()) >= 0 for v in cache.values())
    assert torch.equal(F.max_pool2d(cache["stem"], 3, 2), cache["pool"])
    assert tuple(cache["conv5_3_out"].shape) == (n, 2048, 7, 7)
    fn = lambda xx, dd, **kw: r50_grad(_r50_params(), xx, dd, preprocessed=preprocessed, **kw)
    g_ref, E_rel, E_cos, moved = masked_figures(fn, x, dfeat, cache, TORCH_DT[dtype], mutants, gscale=r50_gscale(dfeat))
    case = "resnet50 %s %dx%d n=%d%s" % (dtype, size[0], size[1], n, " preprocessed" if preprocessed else "")
    _judge(case, g, g_ref, E_rel, E_cos, moved)


def test_reference_is_the_oracle_and_masks_make_it_linear():
    """No GPU (it sits with the tests whose reference it vouches for).  With no masks the two restatements ARE the oracles'
    forwards (float64, to rounding); with the masks of their own forward the masked, folded forms give the same gradient as
    autograd through the ReLUs / PReLUs; and torch's max-pool backward gives a tie to the first maximum."""
    from oracle import ir_resnet, vgg_resnet50 as O
    _threads()
    x, dfeat = _r50_inputs((201, 215), 1, False, seed=3)
    rec = {}
    f, g_plain = r50_grad(_r50_params(), x, dfeat, record=rec, eps=O.BN_EPS)
    want = O.forward(_r50_params(), O.preprocess_input_v2(x), dtype=torch.float64)
    assert np.abs(f - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    _, g_mask = r50_grad(_r50_params(), x, dfeat, masks=rec, eps=O.BN_EPS)
    rel, _ = _rel_cos(g_mask, g_plain)
    print("resnet50: masked reference with its own masks against autograd through the ReLUs: rel %s" % rel)
    assert (rel <= 1e-10).all()
    xp = O.preprocess_input_v2(x)
    _, g_pre = r50_grad(_r50_params(), xp, dfeat, masks=rec, preprocessed=True, eps=O.BN_EPS)
    assert (_rel_cos(g_pre[..., ::-1], g_plain)[0] <= 1e-10).all()
    units = (2, 1, 2, 1)
    p = ir_params(units, True)
    rng = np.random.default_rng(1)
    xi = rng.integers(0, 256, (2, 112, 112, 3)).astype(np.float32)
    dz = rng.standard_normal((2, 512))
    rec = {}
    z, g_plain = ir_grad(p, xi, dz, record=rec, eps=ir_resnet.BN_EPS)
    want = ir_resnet.forward_raw({k: np.asarray(v, np.float64) for k, v in p.items()},
                                 torch.from_numpy(np.transpose(xi, (0, 3, 1, 2)).copy()), dtype=torch.float64).numpy()
    assert np.abs(z - want).max() <= 1e-10 * max(1.0, np.abs(want).max())
    _, g_mask = ir_grad(p, xi, dz, masks=rec, eps=ir_resnet.BN_EPS)
    rel, _ = _rel_cos(g_mask, g_plain)
    print("IR backbone: masked reference with its own masks against autograd through the PReLUs: rel %s" % rel)
    assert (rel <= 1e-10).all()
    t = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    t[0, 0, 0, 2] = t[0, 0, 2, 0] = 1.0
    t.requires_grad_(True)
    F.max_pool2d(t, 3, 2).sum().backward()
    assert t.grad[0, 0, 0, 2] == 1 and t.grad.sum() == 1


@gpu_test
@pytest.mark.parametrize("dtype,size,n,preprocessed", [
    ("bf16", (224, 224), 3, False), ("f16", (224, 224), 3, False),      # today's shapes under the new yardstick
    ("bf16", (201, 215), 2, False), ("f16", (201, 215), 2, False),      # odd x odd: the other stem parity, maps 49/25/13/7 wide
    ("bf16", (224, 199), 2, False), ("f16", (224, 199), 2, False),      # even x odd: non-square maps
    ("f16", (201, 215), 2, True)])                                     # preprocessed input: the stem backward's channel order
def test_resnet50_input_gradient_against_masked_reference(gpu, dtype, size, n, preprocessed):
    _r50_case(gpu, dtype, size, n, preprocessed)


@gpu_test
def test_resnet50_large_batch_takes_the_tile_forms(gpu):
    """34 images: 49 x 34 > 1,600 pixels in the last stage, so every backward convolution runs its tile form (the small batches
    above run the latency forms in stages 4 and 5).  The mutants are a property of the reference and ran above."""
    _r50_case(gpu, "bf16", (224, 224), 34, mutants=[])


@gpu_test
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_resnet50_gradient_is_the_same_bits_without_the_latency_forms(gpu, dtype):
    """The latency forms are documented bit-identical to the tile kernels (include/alink_hip_debug.h; the forward:
    tests/test_gpu_backbone.py): so are the gradients of a 3-image batch with them switched off."""
    lib = gpu.load()
    x, dfeat = _r50_inputs((224, 224), 3, False)
    f1, g1, _ = _r50_gpu(gpu, dtype, (224, 224), x, dfeat, False, want_cache=False)
    lib.alink_debug_set_latency_form(0)
    try:
        f0, g0, _ = _r50_gpu(gpu, dtype, (224, 224), x, dfeat, False, want_cache=False)
    finally:
        lib.alink_debug_set_latency_form(1600)
    assert torch.equal(f0, f1)
    assert np.array_equal(g0, g1), "rel %s" % (_rel_cos(g0, g1)[0],)


@gpu_test
def test_resnet50_widths_the_stem_backward_cannot_take_are_refused_in_words(gpu):
    """Widths 225 .. 228 pass alink_resnet50_create (a 7 x 7 final map) but exceed the stem backward's row tiles: refused at
    alink_resnet50_enable_grad with a message, not by a bare invalid-value after a whole backward pass.  Nothing is run."""
    from a_link_amd.resnet50 import VGGResNet50
    for w in (225, 228):
        with pytest.raises(gpu.AlinkError, match=r"alink_resnet50_enable_grad.*up to 224 pixels wide.*224 x %d" % w):
            VGGResNet50(image_size=(224, w), weights=_r50_params(), dtype="bf16", max_batch=1, enable_grad=True)
    # the forward-only network of that width is still built
    assert not VGGResNet50(image_size=(224, 228), weights=_r50_params(), dtype="bf16", max_batch=1).grad_enabled


# ---- IR backbone cases -------------------------------------------------------------------------------------------------------
def _ir_gpu(gpu, params, dtype, x, demb, nchw, want_cache=True):
    from a_link_amd.backbone import IRBackbone
    n = len(x)
    bb = IRBackbone(params, image_size=(112, 112), dtype=dtype, max_batch=n, enable_grad=True)
    xd = torch.from_numpy(x).cuda()
    if nchw:
        xd = xd.permute(0, 3, 1, 2).contiguous()
    emb = bb.embed_with_cache(xd)
    assert torch.equal(emb, bb.embed_device(xd)), "the cached forward is not the plain forward bit for bit"
    g = bb.input_gradient(torch.from_numpy(demb).cuda())
    if nchw:
        g = g.permute(0, 2, 3, 1)
    cache = _cache(gpu.load(), "alink_debug_backbone_grad_cache_info", bb.h, n, bb.ws.tensor("grad"), TORCH_DT[dtype]) if want_cache else None
    return emb.double().cpu().numpy(), g.contiguous().cpu().numpy(), cache


def _ir_case(gpu, dtype, units, normalized, n, nchw, mutants=True):
    params = ir_params(units, normalized)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (n, 112, 112, 3)).astype(np.float32)
    demb = rng.standard_normal((n, 512)).astype(np.float32)
    e, g, cache = _ir_gpu(gpu, params, dtype, x, demb, nchw)
    assert np.isfinite(e).all() and len(cache) == sum(units) + 2
    norms = cache.pop("norms").numpy()
    assert (norms > 0).all() and tuple(cache["stem"].shape) == (n, 64, 112, 112)
    # the L2 normalisation linearised where the GPU forward stood: d(z) = (g - (g . e) e) / |z| (l2norm_bwd_kernel)
    dz = (demb.astype(np.float64) - (demb * e).sum(1, keepdims=True) * e) / norms[:, None]
    fn = lambda xx, dd, **kw: ir_grad(params, xx, dd, **kw)
    g_ref, E_rel, E_cos, moved = masked_figures(fn, x, dz, cache, TORCH_DT[dtype], ir_mutants(units) if mutants else [])
    case = "ir %s units %s%s n=%d %s" % (dtype, "-".join(str(u) for u in units), " normalized" if normalized else "", n,
                                        "NCHW" if nchw else "NHWC")
    _judge(case, g, g_ref, E_rel, E_cos, moved)


@gpu_test
@pytest.mark.parametrize("dtype,units,normalized,nchw", [
    ("bf16", (2, 2, 2, 2), False, False), ("f16", (2, 2, 2, 2), True, True),
    ("bf16", (3, 4, 14, 3), False, False), ("f16", (3, 4, 14, 3), True, False)])
def test_ir_input_gradient_against_masked_reference(gpu, dtype, units, normalized, nchw):
    """112 x 112, the product's only size: the backward convolutions run the 112-wide direct variant and the linear-tile kernel
    in `dact` mode with non-zero PReLU slopes, which no other test reaches."""
    _ir_case(gpu, dtype, units, normalized, 4, nchw)


@gpu_test
def test_ir_large_batch_takes_the_tile_forms(gpu):
    _ir_case(gpu, "bf16", (2, 2, 2, 2), False, 34, False, mutants=False)


@gpu_test
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_ir_gradient_is_the_same_bits_without_the_latency_forms(gpu, dtype):
    lib = gpu.load()
    params = ir_params((2, 2, 2, 2), True)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (4, 112, 112, 3)).astype(np.float32)
    demb = rng.standard_normal((4, 512)).astype(np.float32)
    e1, g1, _ = _ir_gpu(gpu, params, dtype, x, demb, False, want_cache=False)
    lib.alink_debug_set_latency_form(0)
    try:
        e0, g0, _ = _ir_gpu(gpu, params, dtype, x, demb, False, want_cache=False)
    finally:
        lib.alink_debug_set_latency_form(1600)
    assert np.array_equal(e0, e1)
    assert np.array_equal(g0, g1), "rel %s" % (_rel_cos(g0, g1)[0],)
