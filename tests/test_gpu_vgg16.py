"""GPU: the VGGFace VGG-16 feature model (csrc/vgg16.hip, siamese.FaceVGG16) against the torch-CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_vgg16_features_match_oracle(gpu, tmp_path):
    from a_link_amd import siamese, vgg16 as V
    from oracle import vgg16 as O
    params = V.synthetic_params(2)
    m = siamese.FaceVGG16((224, 224), weights=params, max_batch=2)
    x = np.random.default_rng(0).integers(0, 256, (3, 224, 224, 3)).astype(np.float32)
    got = m.process(x)
    want = O.process(params, x)
    assert got.shape == (3, 25088) and got.dtype == np.float32
    a, b = got.astype(np.float64), want.astype(np.float64)
    cos = 1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    assert cos.max() < 1e-3, cos
    assert (np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max() < 3e-2
    # the reference's call: predict(preprocess(X)) equals the fused raw-pixel path
    pre = m.preprocess(x)
    assert np.array_equal(pre, O.preprocess_input_v1(x))
    assert np.array_equal(m.model.predict(pre), got)
    # Keras weight-file round trip
    path = str(tmp_path / "rcmalli_vggface_tf_notop_vgg16.h5")
    V.save_keras_h5(path, params)
    m2 = siamese.FaceVGG16((224, 224), weights=path)
    assert np.array_equal(m2.process(x[:1]), got[:1])
    assert m.process(np.zeros((0, 224, 224, 3), np.float32)).shape == (0, 25088)


# ---- per-layer parity on the device's own activations ---------------------------------------------------------------------------
# The test above judges 25088 features as one vector, behind five max-pools that each keep one position in four.  The tests below
# stop the forward after every op (alink_debug_vgg16_embed_prefix: alink_vgg16_embed's own loop, cut short), read what the op left
# in the caller's workspace, and judge op i against its float64 reference applied to the device's output of op i - 1
# (tests/vgg16_ref.py; tests/test_vgg16_ref_host.py shows on the CPU that the tolerance holds for a float32 device and that it
# catches a rolled bias, transposed taps, swapped channels, a dropped ReLU, a wrong border, a shifted pool window and a wrong
# flip / mean order).  Parameters: the synthetic kernels with biases of 0.5; images standard normal, fed as preprocessed.
# Every case asserts the kernel and the form each layer reports against a table written here from direct_variant_tiles /
# linear_variant / conv3x3_lat_applies.
#
# Measured on an MI355X, largest err / tol over the convolution layers of a case (the float32 stand-in of the host test: 0.90
# bf16, 0.32 f16 — the device is where a float32 device is, half an ulp of the stored value plus float32 summation):
#   32x32 0.84 bf16 / 0.30 f16;  112x112 0.85 / 0.29 (the same with the latency form off);  56x112 0.89 / 0.29 (the same with
#   the pair kernels off);  74x100 0.85 / 0.30;  224x224 0.90 bf16;  raw pixels through the stem (s = 105): 0.82 / 0.33.
# End to end against oracle/vgg16.process on raw pixels, worst size: 1 - cos 2.7e-5, relative L2 7.4e-3 (bf16); 4.5e-7, 9.7e-4 (f16).
import ctypes as C

import torch

import vgg16_ref as R
from test_gpu_conv_forms import restore

# ConvKernel (a-link_amd/csrc/conv_kernel.h) and forms (0 = the kernel itself, 1 = conv3x3_lat_kernel)
IGEMM, T14C256, T28C256, T28C128, T56C128, T56C64, T112C64, P14, P28 = 0, 1, 2, 3, 4, 5, 6, 7, 8
L14, L28, L56, L7 = 11, 12, 13, 14
LINEAR = (L14, L28, L56, L7)
SELF, LAT = 0, 1
CONVS = [name for kind, name in R.OPS if kind == "conv"]          # conv1_2 .. conv5_3: 1 + 2 + 3 + 3 + 3


def _table(b1, b2, b3, b4, b5):
    """(kernel, form) of conv1_2 and of every layer of blocks 2..5"""
    rows = [b1] + [b2] * 2 + [b3] * 3 + [b4] * 3 + [b5] * 3
    return dict(zip(CONVS, rows))


def _g(k):
    return (k, SELF)


# name -> size (H, W), images, max_batch, switches set before the network is built, dtypes, expected (kernel, form) per layer
CASES = {
    # every layer on the implicit GEMM, down to a 2 x 2 map at 512 channels; three images in chunks of two and one
    "32x32": dict(size=(32, 32), n=3, max_batch=2, sw={}, dts=("bf16", "f16"), table=_table(*[_g(IGEMM)] * 5)),
    # square maps 56 / 28 / 14 / 7: the linear-tile kernels; two images are 1568, 392, 98 pixels at 28, 14, 7 wide: the
    # latency form (<= 1600 pixels, Cin >= 128, <= 448 waves) serves blocks 3..5, the 56-wide block (6272 pixels) is Linear56
    "112x112": dict(size=(112, 112), n=2, max_batch=2, sw={}, dts=("bf16", "f16"),
                    table=_table(_g(T112C64), _g(L56), (L28, LAT), (L14, LAT), (L7, LAT))),
    "112x112-nolat": dict(size=(112, 112), n=2, max_batch=2, sw=dict(latency_form=0), dts=("bf16", "f16"),
                          table=_table(_g(T112C64), _g(L56), _g(L28), _g(L14), _g(L7))),
    # not square: no linear tiles.  112 wide at H = 56, then 56 / 28 / 14 wide tile and pair kernels at Cin 64 .. 512, then a
    # 3 x 7 map (GEMM) pooled to 1 x 3
    "56x112": dict(size=(56, 112), n=2, max_batch=2, sw={}, dts=("bf16", "f16"),
                   table=_table(_g(T112C64), _g(T56C128), _g(P28), _g(P14), _g(IGEMM))),
    "56x112-nopair": dict(size=(56, 112), n=2, max_batch=2, sw=dict(pair=0), dts=("bf16", "f16"),
                          table=_table(_g(T112C64), _g(T56C128), _g(T28C256), _g(T14C256), _g(IGEMM))),
    # the stem at a width that is no multiple of 16 and a height that is no multiple of its 8-row band; tile kernels at widths
    # 50, 25, 12; pools of 37 x 50, 18 x 25 and 9 x 12 maps (odd height, width, height)
    "74x100": dict(size=(74, 100), n=2, max_batch=2, sw={}, dts=("bf16", "f16"),
                   table=_table(_g(IGEMM), _g(T56C128), _g(P28), _g(P14), _g(IGEMM))),
    # the reference's own size, one image: the GEMM at width 224; 112 wide TileW112C64 at Cin 64 and the GEMM at Cin 128 (two
    # input buffers of the 112-wide tile do not fit the LDS); Linear56 at Cin 128 / 256 (3136 pixels: its own form), Linear28
    # at Cin 256 / 512 and Linear14 in the latency form (784 and 196 pixels)
    "224x224": dict(size=(224, 224), n=1, max_batch=1, sw={}, dts=("bf16",),
                    table=dict(_table(_g(IGEMM), _g(T112C64), _g(L56), (L28, LAT), (L14, LAT)), conv2_2=_g(IGEMM))),
}
# one family (size) and type after the other: the settings of a family share their references
PARITY = [(c, dt) for fam in dict.fromkeys(c.split("-")[0] for c in CASES) for dt in ("bf16", "f16")
          for c in CASES if c.split("-")[0] == fam and dt in CASES[c]["dts"]]
TDT = R.TORCH_DT
_PARAMS, _NETS, _REFS, _DONE = {}, {}, {"key": None, "refs": {}}, {}


def _params():
    if not _PARAMS:
        _PARAMS.update(R.draw_params(21))
    return _PARAMS


def _net(size, dt, max_batch, fresh=False):
    """a FaceVGG16 on the drawn parameters; cached unless a switch that acts at finalize is set (fresh)"""
    from a_link_amd import siamese
    key = (size, dt, max_batch)
    if fresh:
        return siamese.FaceVGG16(size, weights=_params(), dtype=dt, max_batch=max_batch)
    if key not in _NETS:
        _NETS[key] = siamese.FaceVGG16(size, weights=_params(), dtype=dt, max_batch=max_batch)
    return _NETS[key]


def _set(lib, sw):
    if "pair" in sw:
        lib.alink_debug_set_pair(sw["pair"])
    if "latency_form" in sw:
        lib.alink_debug_set_latency_form(sw["latency_form"])


def _prefix(gpu, m, x, n_ops, preprocessed):
    """the first n_ops ops on x (a float32 device tensor), in embed_device's chunks of max_batch.  Returns (out, name, reports):
    out the CPU copy of what op n_ops - 1 wrote, (n, H, W, C) in the handle's type — float32 for the last pool —, and
    reports [(kernel, form)] per chunk"""
    net, lib = m.model, gpu.load()
    fn = lib.alink_debug_vgg16_embed_prefix
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                   C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int,
                   C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert fn(net.h, None, 0, 0, None, None, 0, None, 0, None, None, None, None, None, 0, None, None) == len(R.OPS)
    last = n_ops == len(R.OPS)
    outs, reports, name = [], [], None
    for i in range(0, x.shape[0], net.max_batch):
        xc = x[i:i + net.max_batch].contiguous()
        n = xc.shape[0]
        ws, wsb = net.ws.get(n)
        feat = torch.empty((n, net.feature_size), dtype=torch.float32, device=x.device) if last else None
        off, H, W, Ch, kern, form = C.c_size_t(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        buf = C.create_string_buffer(32)
        rc = fn(net.h, gpu.ptr(xc), n, 1 if preprocessed else 0, gpu.ptr(feat), ws, wsb, gpu.current_stream(net.device), n_ops,
                C.byref(off), C.byref(H), C.byref(W), C.byref(Ch), buf, 32, C.byref(kern), C.byref(form))
        assert rc == len(R.OPS), lib.alink_last_error()
        torch.cuda.synchronize()
        shape = (n, H.value, W.value, Ch.value)
        if last:
            out = feat.cpu().reshape(shape)
        else:
            t = net.ws.tensor()
            at = ws - t.data_ptr() + off.value
            out = t[at:at + 2 * int(np.prod(shape))].clone().view(TDT[net.dtype]).reshape(shape).cpu()
        outs.append(out)
        reports.append((kern.value, form.value))
        assert name in (None, buf.value.decode())
        name = buf.value.decode()
    return torch.cat(outs), name, reports


def _reference(key, i, dt, A):
    """op i's reference and tolerance on A; kept while the same case family (size, type) runs, so that a second setting of the
    switches, which must give the same bits, does not pay for the float64 convolutions again"""
    if _REFS["key"] != key:
        _REFS["key"], _REFS["refs"] = key, {}
    h = (i, hash(A.numpy().tobytes()))
    if h not in _REFS["refs"]:
        ref, Wt = R.op_ref(_params(), dt, i, A)
        _REFS["refs"][h] = (ref, None if Wt is None else R.tolerance(ref, A, Wt, dt))
    return _REFS["refs"][h]


def _judge_chain(gpu, m, x, dt, preprocessed, table, label, linear_ok=True):
    """every prefix of the forward on x; returns ([op outputs as the device left them], {(kernel, form)} reported)"""
    A = R.stem_pixels(x.cpu().numpy(), dt, preprocessed)
    outs, seen = [], set()
    for i, (kind, name) in enumerate(R.OPS):
        got, gname, reports = _prefix(gpu, m, x, i + 1, preprocessed)
        assert gname == name, (label, i, gname)
        ref, tol = _reference((label.split("-")[0], dt, preprocessed), i, dt, A)
        assert tuple(got.shape) == tuple(R.nhwc(ref).shape), (label, name, got.shape)
        g64 = R.nchw(got.double())
        if kind == "pool":
            assert reports == [(-1, 0)] * len(reports)
            assert got.dtype == (torch.float32 if i + 1 == len(R.OPS) else TDT[dt])
            assert torch.equal(g64, ref), "%s %s: the pool is not the exact maximum" % (label, name)
            print("%s %s %s %dx%d: exact" % (label, dt, name, ref.shape[2], ref.shape[3]))
        else:
            assert torch.isfinite(g64).all(), (label, name)
            w = R.worst(g64, ref, tol)
            print("%s %s %s %dx%d Cin %d: kernel %s form %s  err/tol %.3f" % (
                label, dt, name, ref.shape[2], ref.shape[3], A.shape[1], reports[0][0] if kind == "conv" else "stem", reports[0][1], w))
            if kind == "stem":
                assert reports == [(-1, 0)] * len(reports)
            elif linear_ok or table[name][0] not in LINEAR:
                assert reports == [table[name]] * len(reports), "%s %s reports (kernel, form) %s, expected %s" % (label, name, reports, table[name])
                seen.update(reports)
            assert w <= 1.0, "%s %s %s: err / tol %.3f" % (label, dt, name, w)
        outs.append(got)
        A = g64
    feat = m.model.embed_device(x, preprocessed).cpu()
    assert torch.equal(outs[-1].reshape(feat.shape), feat), "%s: prefix 18 is not embed_device bit for bit" % label
    return outs, seen


def _images(seed, n, size):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n,) + size + (3,)).astype(np.float32)).cuda()


def _run_case(gpu, case, dt):
    """the per-layer parity of one case; its reported (kernel, form) set.  Done once per process (the coverage test asks again)."""
    if (case, dt) in _DONE:
        return _DONE[case, dt]
    c, lib = CASES[case], gpu.load()
    linear_ok = lib.alink_debug_linear_contract_ok() == 1
    try:
        _set(lib, c["sw"])
        m = _net(c["size"], dt, c["max_batch"], fresh="pair" in c["sw"])
        assert m.model.feature_size == (c["size"][0] >> 5) * (c["size"][1] >> 5) * 512
        _, seen = _judge_chain(gpu, m, _images(3, c["n"], c["size"]), dt, True, c["table"], case, linear_ok)
    finally:
        restore(lib)
    _DONE[case, dt] = (seen, linear_ok)
    return _DONE[case, dt]


@pytest.mark.parametrize("case,dt", PARITY)
def test_vgg16_per_layer_parity(gpu, case, dt):
    """Every op of the forward against its float64 reference on the device's own input of that op; the kernel and form of
    every layer against the case's table.  Prints, per layer, the kernel, the form and the largest err / tol (-s); the
    measured figures are in the comment above."""
    _run_case(gpu, case, dt)


def test_vgg16_cases_cover_every_kernel(gpu):
    seen, linear_ok = set(), True
    for case, dt in PARITY:
        s, ok = _run_case(gpu, case, dt)
        seen |= s
        linear_ok = linear_ok and ok
    want = [_g(IGEMM), _g(T112C64), _g(T56C128), _g(T28C256), _g(P28), _g(T14C256), _g(P14)]
    if linear_ok:
        want += [_g(L56), _g(L28), _g(L14), _g(L7)]
        assert any(f == LAT for _, f in seen), seen
    missing = [kf for kf in want if kf not in seen]
    assert not missing, "no case ran (kernel, form) %s; ran %s" % (missing, sorted(seen))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_vgg16_raw_pixel_path(gpu, dt):
    """Integer pixels through the stem's flip / means loader (preprocessed=False) at 74 x 100: op 0 against the stem reference,
    and the whole chain bit-equal to the run on host-preprocessed pixels."""
    from oracle import vgg16 as O
    size = (74, 100)
    m = _net(size, dt, 2)
    x = np.random.default_rng(4).integers(0, 256, (2,) + size + (3,)).astype(np.float32)
    xd, pre = torch.from_numpy(x).cuda(), torch.from_numpy(O.preprocess_input_v1(x)).cuda()
    got, name, _ = _prefix(gpu, m, xd, 1, False)
    A = R.stem_pixels(x, dt, False)
    ref, Wt = R.op_ref(_params(), dt, 0, A)
    w = R.worst(R.nchw(got.double()), ref, R.tolerance(ref, A, Wt, dt))
    print("raw pixels %s conv1_1: s = %s err/tol %.3f" % (dt, R.scale(A, Wt).flatten().tolist(), w))
    assert name == "conv1_1" and torch.isfinite(got.double()).all() and w <= 1.0, w
    for n_ops in range(1, len(R.OPS) + 1):
        a, b = _prefix(gpu, m, xd, n_ops, False)[0], _prefix(gpu, m, pre, n_ops, True)[0]
        assert a.dtype == b.dtype and torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                                                  b.view(torch.int32 if a.dtype == torch.float32 else torch.int16)), n_ops
    assert torch.equal(m.model.embed_device(xd, False), m.model.embed_device(pre, True))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_vgg16_non_finite_stays_in_its_image(gpu, dt):
    """NaN at two corner pixels of image 1 of three: images 0 and 2 keep every bit at every op, image 1 is non-finite exactly
    where the reference is, and its features hold NaN (nothing is flushed to zero)."""
    size = (74, 100)
    m = _net(size, dt, 3)
    clean = _images(8, 3, size)
    x = clean.clone()
    x[1, 0, 0, :] = float("nan")
    x[1, size[0] - 1, size[1] - 1, :] = float("nan")
    bits = lambda t: t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    A = R.stem_pixels(x[1:2].cpu().numpy(), dt, True)
    for i, (kind, name) in enumerate(R.OPS):
        got = _prefix(gpu, m, x, i + 1, True)[0]
        ok = _prefix(gpu, m, clean, i + 1, True)[0]
        assert torch.equal(bits(got[0]), bits(ok[0])) and torch.equal(bits(got[2]), bits(ok[2])), "%s: a neighbour image changed" % name
        ref, _ = R.op_ref(_params(), dt, i, A)
        g1 = R.nchw(got[1:2].double())
        assert torch.equal(torch.isfinite(g1), torch.isfinite(ref)), "%s: %d non-finite outputs, the reference has %d" % (
            name, int((~torch.isfinite(g1)).sum()), int((~torch.isfinite(ref)).sum()))
        assert (~torch.isfinite(g1)).any(), name
        print("non-finite %s %s: %d of %d outputs of image 1" % (dt, name, int((~torch.isfinite(g1)).sum()), g1.numel()))
        A = g1
    feat = m.model.embed_device(x, True).cpu()
    assert torch.isnan(feat[1]).any() and torch.isfinite(feat[0]).all() and torch.isfinite(feat[2]).all()


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("size,n,max_batch", [((32, 32), 3, 2), ((112, 112), 2, 2), ((56, 112), 2, 2), ((74, 100), 2, 2)])
def test_vgg16_features_match_oracle_at_every_size(gpu, size, n, max_batch, dt):
    from oracle import vgg16 as O
    m = _net(size, dt, max_batch)
    x = np.random.default_rng(9).integers(0, 256, (n,) + size + (3,)).astype(np.float32)
    got, want = m.process(x), O.process(_params(), x)
    assert m.model.feature_size == (size[0] >> 5) * (size[1] >> 5) * 512
    assert got.shape == want.shape == (n, m.model.feature_size) and got.dtype == np.float32
    a, b = got.astype(np.float64), want.astype(np.float64)
    cos = 1 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    print("%s %s: 1 - cos %.2e, relative L2 %.2e" % (size, dt, cos.max(), rel.max()))
    assert cos.max() < 1e-3, cos
    assert rel.max() < 3e-2, rel


def test_vgg16_api_refuses_bad_sizes_and_shapes(gpu):
    from a_link_amd import siamese
    for size in [(16, 64), (64, 31), (544, 64), (64, 513)]:
        with pytest.raises(gpu.AlinkError):
            siamese.FaceVGG16(size, weights=_params())
    m = _net((32, 32), "bf16", 2)
    for shape in [(1, 32, 33, 3), (1, 32, 32, 4), (32, 32, 3)]:
        with pytest.raises(ValueError):
            m.process(np.zeros(shape, np.float32))
