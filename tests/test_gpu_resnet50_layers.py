"""GPU: every op of the VGGFace2 ResNet-50 forward (csrc/resnet50.hip) against its one-op float64 reference, in bf16, f16 and
split precision (f16x2), at sizes off 224 x 224.

tests/test_gpu_resnet50.py judges the 2048 features as one vector, behind a 7 x 7 average, sixteen residual sums and a
max-pool.  The tests below stop the forward after every op (alink_debug_resnet50_embed_prefix: r50_run's own loop, cut short),
read what the op left in the caller's workspace, and judge op i against its reference applied to the device's own outputs of
the ops it reads — input and residual (tests/resnet50_ref.py; tests/test_resnet50_ref_host.py shows on the CPU that the
tolerances hold for a float32 device and that they catch a rolled bias, swapped channels, transposed taps, a dropped ReLU or
post_relu, a dropped or misread residual, a stride-2 1x1 on odd positions, a swapped stem pad, a shifted pool window, a wrong
divisor and a wrong flip / mean order).  Parameters: resnet50_ref.draw_params (betas and means of 0.5); images standard normal,
fed as preprocessed.  Every case asserts the name, shape, kernel and form each op reports against a table written here from
direct_variant_tiles / linear_variant_x2 / conv3x3_lat_applies / conv_gemm_lat_applies (restated as rules in
resnet50_ref.expected_table; tests/test_resnet50_ref_host.py compares the two).

The max-pool of a 112-wide stem map is 55 wide ('valid', 3 / 2), so at 224 x 224 stage 2 is NOT a linear-tile width: it takes
TileW56C64 (16-bit) or the implicit GEMM (split precision).  Linear56 arises only for 225 .. 228 (a 113- or 114-wide stem map):
the 228x228 case.

Measured on an MI355X, largest err / tol over the ops of a kind, all seven cases (the float32 stand-in of the host test: 0.93
bf16, 0.39 f16, 0.14 f16x2 for the convolutions — the device is where a float32 device is):
            stem    1x1     3x3     average pool   max-pool
  bf16      0.87    0.93    0.87    0.03           exact
  f16       0.32    0.40    0.31    0.04           exact
  f16x2     0.05    0.07    0.09    0.15           exact (hi + lo has at most 22 bits)
Every table row as written; prefix 55 bit-equal to embed_device; latency form off bit-equal to on at every op.  No defect found.
That the test can fail: with the reference of conv2_3_1x1_increase reading its residual from conv2_1's output (a scratch change on
the CPU side, not kept), the device is reported at exactly that op, err / tol 922.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import resnet50_ref as R
from test_gpu_conv_forms import restore

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))          # the float64 references are CPU work

NOPS = len(R.OPS)
IGEMM, T56C64, P14, P28, L14, L28, L56, L7 = R.IGEMM, R.T56C64, R.P14, R.P28, R.L14, R.L28, R.L56, R.L7
SELF, LAT3, LATG = R.SELF, R.LAT3, R.LATG
# the 1x1 layers conv_gemm_lat_kernel serves (Cin 64 .. 512, at most 784 pixels and 512 waves) for ONE image per launch ...
LONE = tuple("conv3_%d_1x1_reduce" % u for u in (1, 2, 3, 4)) + ("conv4_1_1x1_reduce",) + tuple("conv5_%d_1x1_increase" % u for u in (1, 2, 3))
PAIR = ("conv4_1_1x1_reduce",)            # ... and for two (392 pixels at 14 x 14; two 28 x 28 maps are 1568, two 7 x 7 x 2048 are 896 waves)


def _t(c2, c3, c4, c5, latg):
    """the (kernel, form) of the 3x3 of stages conv2 .. conv5, and the names of the 1x1 layers in the GEMM latency form (every
    other 1x1 is (IGEMM, SELF))"""
    return dict(conv2=c2, conv3=c3, conv4=c4, conv5=c5, latg=latg)


# name -> size, images, max_batch (images per launch), latency switch, {type class: table}.  "16": bf16 and f16; "x2": f16x2,
# which has the linear-tile kernels and the implicit GEMM only
CASES = {
    # one image: 55-wide stage 2 on the row-aligned tile kernel; the 28-, 14- and 7-wide 3x3 (784, 196, 49 pixels) in the latency form
    "224x224-n1": dict(size=(224, 224), n=1, mb=1, lat=None,
                       t16=_t((T56C64, SELF), (L28, LAT3), (L14, LAT3), (L7, LAT3), LONE),
                       tx2=_t((IGEMM, SELF), (L28, LAT3), (L14, LAT3), (L7, LAT3), LONE)),
    # two images, default switches: 1568 pixels at 28 wide are still the latency form
    "224x224-n2": dict(size=(224, 224), n=2, mb=2, lat=None,
                       t16=_t((T56C64, SELF), (L28, LAT3), (L14, LAT3), (L7, LAT3), PAIR),
                       tx2=_t((IGEMM, SELF), (L28, LAT3), (L14, LAT3), (L7, LAT3), PAIR)),
    # ... and with the latency forms off: the linear-tile kernels themselves at every width, bit-identical to the case above
    "224x224-n2-nolat": dict(size=(224, 224), n=2, mb=2, lat=0,
                             t16=_t((T56C64, SELF), (L28, SELF), (L14, SELF), (L7, SELF), ()),
                             tx2=_t((IGEMM, SELF), (L28, SELF), (L14, SELF), (L7, SELF), ())),
    # stem pad 3/3 over 2/3, 99 stem rows (no multiple of 4) x 114 columns (no multiple of 16); maps 49 x 56, 25 x 28, 13 x 14: no
    # linear tiles before the 7 x 7 map; two images in two launches
    "197x228": dict(size=(197, 228), n=2, mb=1, lat=None,
                    t16=_t((T56C64, SELF), (P28, SELF), (P14, SELF), (L7, LAT3), LONE),
                    tx2=_t((IGEMM, SELF), (IGEMM, SELF), (IGEMM, SELF), (L7, LAT3), LONE)),
    # odd widths 99, 49, 25, 13
    "228x197": dict(size=(228, 197), n=1, mb=1, lat=None,
                    t16=_t((T56C64, SELF), (P28, SELF), (P14, SELF), (L7, LAT3), LONE),
                    tx2=_t((IGEMM, SELF), (IGEMM, SELF), (IGEMM, SELF), (L7, LAT3), LONE)),
    # square maps 52, 26, 13: square, but no linear-tile widths
    "211x211": dict(size=(211, 211), n=1, mb=1, lat=None,
                    t16=_t((T56C64, SELF), (P28, SELF), (P14, SELF), (L7, LAT3), LONE),
                    tx2=_t((IGEMM, SELF), (IGEMM, SELF), (IGEMM, SELF), (L7, LAT3), LONE)),
    # the largest size: a 114-wide stem map pooled to 56: Linear56 in its own form (3136 pixels, Cin 64)
    "228x228": dict(size=(228, 228), n=1, mb=1, lat=None,
                    t16=_t((L56, SELF), (L28, LAT3), (L14, LAT3), (L7, LAT3), LONE),
                    tx2=_t((L56, SELF), (L28, LAT3), (L14, LAT3), (L7, LAT3), LONE)),
}
PARITY = [(c, dt) for dt in R.TYPES for c in CASES]
# every (type class, kernel, form, kernel size) a layer of this network takes at sizes 197 .. 228 with one or two images per launch
COVER = [(tc, IGEMM, SELF, 1) for tc in ("16", "x2")] + [(tc, IGEMM, LATG, 1) for tc in ("16", "x2")] + \
        [("x2", IGEMM, SELF, 3), ("16", T56C64, SELF, 3), ("16", P28, SELF, 3), ("16", P14, SELF, 3)]
COVER_LINEAR = [(tc, k, f, 3) for tc in ("16", "x2") for k, f in ((L56, SELF), (L28, SELF), (L28, LAT3), (L14, SELF), (L14, LAT3),
                                                                   (L7, SELF), (L7, LAT3))]


def table_rows(case, dt):
    """[(kernel, form)] per op from the case's table"""
    t = CASES[case]["tx2" if dt == "f16x2" else "t16"]
    rows = []
    for op in R.OPS:
        if op.kind != "conv":
            rows.append((-1, 0))
        elif op.k == 3:
            rows.append(t[op.name[:5]])
        else:
            rows.append((IGEMM, LATG if op.name in t["latg"] else SELF))
    return rows


_PARAMS, _NETS, _REFS, _DONE, _WORST = {}, {}, {"key": None, "refs": {}}, {}, {}


def _params():
    if not _PARAMS:
        _PARAMS.update(R.draw_params(21))
    return _PARAMS


def _net(size, dt, mb):
    from a_link_amd.resnet50 import VGGResNet50
    key = (size, dt, mb)
    if key not in _NETS:
        _NETS[key] = VGGResNet50(size, weights=_params(), dtype=dt, max_batch=mb)
    return _NETS[key]


def _calibrate(gpu, m, x, preprocessed):
    """split precision: the scales from x itself, all of it in ONE launch chain (whatever max_batch is)"""
    lib, n = gpu.load(), x.shape[0]
    ws, wsb = m.ws.get(n)
    torch.cuda.synchronize()
    gpu.check(lib.alink_resnet50_calibrate(m.h, gpu.ptr(x), n, 1 if preprocessed else 0, ws, wsb, 0, gpu.current_stream(m.device)),
              "alink_resnet50_calibrate")


def _fn(gpu):
    fn = gpu.load().alink_debug_resnet50_embed_prefix
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                   C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int,
                   C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return fn


def _prefix(gpu, m, x, n_ops, preprocessed):
    """the first n_ops ops on x (a float32 device tensor), in embed_device's chunks of max_batch.  Returns (raw, name, reports, e):
    raw the CPU copy of what op n_ops - 1 wrote — (n, H, W, C) in the handle's 16-bit type, (n, H, W, 2 C) float16 in split
    precision, (n, 1, 1, 2048) float32 for the average pool —, reports [(kernel, form)] per chunk, e the reported exponent"""
    fn, lib = _fn(gpu), gpu.load()
    assert fn(m.h, None, 0, 0, None, None, 0, None, 0, None, None, None, None, None, 0, None, None, None) == NOPS
    last, x2 = n_ops == NOPS, m.dtype == "f16x2"
    outs, reports, name, exps = [], [], None, set()
    for i in range(0, x.shape[0], m.max_batch):
        xc = x[i:i + m.max_batch].contiguous()
        n = xc.shape[0]
        ws, wsb = m.ws.get(n)
        feat = torch.full((n, 2048), 7.0, dtype=torch.float32, device=x.device)
        off, H, W, Ch, kern, form, e = C.c_size_t(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        buf = C.create_string_buffer(48)
        rc = fn(m.h, gpu.ptr(xc), n, 1 if preprocessed else 0, gpu.ptr(feat) if last else None, ws, wsb, gpu.current_stream(m.device),
                n_ops, C.byref(off), C.byref(H), C.byref(W), C.byref(Ch), buf, 48, C.byref(kern), C.byref(form), C.byref(e))
        assert rc == NOPS, lib.alink_last_error()
        torch.cuda.synchronize()
        if last:
            assert (H.value, W.value, Ch.value, off.value) == (1, 1, 2048, 0)
            out = feat.cpu().reshape(n, 1, 1, 2048)
        else:
            shape = (n, H.value, W.value, Ch.value * (2 if x2 else 1))
            t = m.ws.tensor()
            at = ws - t.data_ptr() + off.value
            assert at + 2 * int(np.prod(shape)) <= t.numel()
            out = t[at:at + 2 * int(np.prod(shape))].clone().view(torch.float16 if x2 else R.TORCH_DT[m.dtype]).reshape(shape).cpu()
        outs.append(out)
        reports.append((kern.value, form.value))
        exps.add(e.value)
        assert name in (None, buf.value.decode())
        name = buf.value.decode()
    assert len(exps) == 1
    return torch.cat(outs), name, reports, exps.pop()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _widen(raw, dt, e, C_):
    """the device's tensor as float64 (n, C, H, W) in true units; split precision also returns hi + lo in stored units"""
    if dt == "f16x2" and raw.dtype == torch.float16:
        hi, lo = R.widen_pairs(raw, C_)
        stored = R.nchw(hi + lo)
        return stored * 2.0 ** -e, stored
    return R.nchw(raw.double()), None


def _reference(key, i, dt, A, Rs):
    """op i's reference and tolerance on A (and Rs); kept while the same case family (size, images, type) runs, so that a second
    setting of the switches, which must give the same bits, does not pay for the float64 convolutions again"""
    if _REFS["key"] != key:
        _REFS["key"], _REFS["refs"] = key, {}
    h = (i, hash(A.numpy().tobytes()), None if Rs is None else hash(Rs.numpy().tobytes()))
    if h not in _REFS["refs"]:
        op = R.OPS[i]
        ref, Wt, bias = R.op_ref(_params(), dt, i, A, Rs)
        tol = R.conv_tolerance(op, dt, ref, A, Wt, bias, Rs) if Wt is not None else None
        _REFS["refs"][h] = (ref, tol)
    return _REFS["refs"][h]


def _note(dt, kind, w):
    _WORST[dt, kind] = max(_WORST.get((dt, kind), 0.0), w)


def _judge_chain(gpu, m, x, dt, preprocessed, rows, label, family, linear_ok=True, judge_upto=NOPS):
    """every prefix of the forward on x; op i < judge_upto against its reference and its table row.  Returns ([raw outputs as the
    device left them], {(kernel, form, kernel size)} reported)"""
    x2 = dt == "f16x2"
    scales = m.state()["scale_exponents"] if x2 else None
    dims = R.shapes(*m.image_size)
    raws, vals, seen = [], [], set()
    for i, op in enumerate(R.OPS):
        raw, name, reports, e = _prefix(gpu, m, x, i + 1, preprocessed)
        raws.append(raw)
        assert name == op.name, (label, i, name)
        last = i + 1 == NOPS
        assert tuple(raw.shape) == (x.shape[0], dims[i][2], dims[i][3], op.cout * (2 if x2 and not last else 1)), (label, name, raw.shape)
        assert raw.dtype == (torch.float32 if last else (torch.float16 if x2 else R.TORCH_DT[dt])), (label, name, raw.dtype)
        val, stored = _widen(raw, dt, e, op.cout)
        vals.append(val)
        if i >= judge_upto:
            continue
        A = R.stem_pixels(x.cpu().numpy(), dt, preprocessed) if op.src is None else vals[op.src]
        Rs = None if op.res is None else vals[op.res]
        ref, tol = _reference((family, dt, preprocessed), i, dt, A, Rs)
        assert torch.isfinite(val).all(), (label, name)
        if x2 and not last:
            # calibration (ScaleCalibration::settle) leaves the largest stored half of a convolution's output in [2^10, 2^11) on
            # the images it ran on — these; the max-pool keeps the stem's exponent (and at most its maximum); no half is non-finite
            assert torch.isfinite(raw.float()).all(), (label, name)
            big = float(raw.float().abs().max())
            assert e == (scales[0] if op.kind == "maxpool" else scales[i]), (label, name, e)
            assert big < 2048.0 and (op.kind == "maxpool" or big >= 1024.0), "%s %s: largest stored half %g at exponent %d" % (label, name, big, e)
        if op.kind == "maxpool":
            if x2:
                ref_s = ref * 2.0 ** e
                w = R.worst(stored, ref_s, R.maxpool_x2_tolerance(ref_s))
                assert w <= 1.0, "%s %s %s: err / tol %.3f" % (label, dt, name, w)
            else:
                w = 0.0
                assert torch.equal(val, ref), "%s %s: the pool is not the exact maximum" % (label, name)
        elif op.kind == "avgpool":
            w = R.worst(val, ref, R.avgpool_tolerance(A))
        else:
            w = R.worst(val, ref, tol)
        _note(dt, op.kind if op.kind != "conv" else "%dx%d" % (op.k, op.k), w)
        print("%s %s %s %dx%d: kernel %d form %d%s  err/tol %.3f" % (label, dt, name, dims[i][2], dims[i][3], reports[0][0], reports[0][1],
                                                                      "  e %d" % e if x2 else "", w))
        if op.kind != "conv":
            assert reports == [(-1, 0)] * len(reports), (label, name, reports)
        elif linear_ok or rows[i][0] not in R.LINEAR:
            assert reports == [rows[i]] * len(reports), "%s %s reports (kernel, form) %s, expected %s" % (label, name, reports, rows[i])
            seen.update((k, f, op.k) for k, f in reports)
        assert w <= 1.0, "%s %s %s: err / tol %.3f" % (label, dt, name, w)
    return raws, seen


def _images(seed, n, size):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n,) + size + (3,)).astype(np.float32)).cuda()


def _run_case(gpu, case, dt):
    """the per-op parity of one case; (its reported (kernel, form, size) set, linear_ok, raw outputs).  Done once per process."""
    if (case, dt) in _DONE:
        return _DONE[case, dt]
    c, lib = CASES[case], gpu.load()
    linear_ok = lib.alink_debug_linear_contract_ok() == 1
    m = _net(c["size"], dt, c["mb"])
    x = _images(3, c["n"], c["size"])
    try:
        if c["lat"] is not None:
            lib.alink_debug_set_latency_form(c["lat"])
        if dt == "f16x2":
            _calibrate(gpu, m, x, True)
        raws, seen = _judge_chain(gpu, m, x, dt, True, table_rows(case, dt), case, (c["size"], c["n"]), linear_ok)
        feat = m.embed_device(x, True).cpu()
        assert torch.equal(_bits(raws[-1].reshape(feat.shape)), _bits(feat)), "%s: prefix 55 is not embed_device bit for bit" % case
        if not any(k[1] == dt for k in _DONE):
            # determinism, asserted once per type: a prefix run again leaves the same bits (what lets op i's reference read the
            # outputs of earlier prefix runs)
            for n_ops in (1, 2, 17, 30, NOPS):
                again = _prefix(gpu, m, x, n_ops, True)[0]
                assert torch.equal(_bits(again), _bits(raws[n_ops - 1])), (case, dt, n_ops)
        torch.cuda.synchronize()
        assert lib.alink_resnet50_range_flag(m.h, 0) == 0, "%s %s: the range flag is up" % (case, dt)
    finally:
        restore(lib)
    _DONE[case, dt] = (seen, linear_ok, raws)
    if case == "224x224-n2-nolat":
        assert _DONE.get(("224x224-n2", dt)) is not None, "the default-switch case runs first"
    return _DONE[case, dt]


@pytest.mark.parametrize("case,dt", PARITY)
def test_resnet50_per_op_parity(gpu, case, dt):
    """Every op of the forward against its float64 reference on the device's own inputs of that op; name, shape, kernel and form
    of every op against the case's table.  Prints, per op, the kernel, the form and the largest err / tol (-s)."""
    raws = _run_case(gpu, case, dt)[2]
    if case == "224x224-n2-nolat":
        # the linear-tile kernels' own forms against the latency forms: every op's output bit for bit
        base = _run_case(gpu, "224x224-n2", dt)[2]
        for i, (a, b) in enumerate(zip(raws, base)):
            assert torch.equal(_bits(a), _bits(b)), "%s: latency form off changes %s" % (dt, R.OPS[i].name)


def test_resnet50_cases_cover_every_kernel(gpu):
    seen, linear_ok = set(), True
    for case, dt in PARITY:
        s, ok, _ = _run_case(gpu, case, dt)
        seen |= {("x2" if dt == "f16x2" else "16",) + kf for kf in s}
        linear_ok = linear_ok and ok
    missing = [kf for kf in COVER + (COVER_LINEAR if linear_ok else []) if kf not in seen]
    assert not missing, "no case ran (type class, kernel, form, size) %s; ran %s" % (missing, sorted(seen))
    for (dt, kind), w in sorted(_WORST.items()):
        print("largest err / tol, %s %s: %.3f" % (dt, kind, w))


@pytest.mark.parametrize("dt", R.TYPES)
def test_resnet50_raw_pixel_path(gpu, dt):
    """Integer pixels through the stem's flip / means loader (preprocessed=False) at 197 x 228: op 0 against the stem reference,
    and every op bit-equal to the run on host-preprocessed pixels."""
    size = (197, 228)
    m, lib = _net(size, dt, 2), gpu.load()
    x = np.random.default_rng(4).integers(0, 256, (2,) + size + (3,)).astype(np.float32)
    from oracle import vgg_resnet50 as O
    xd, pre = torch.from_numpy(x).cuda(), torch.from_numpy(O.preprocess_input_v2(x)).cuda()
    try:
        if dt == "f16x2":
            _calibrate(gpu, m, xd, False)
        raws, _ = _judge_chain(gpu, m, xd, dt, False, None, "raw pixels", (size, 2, "raw"), judge_upto=1)
        for n_ops in range(1, NOPS + 1):
            b = _prefix(gpu, m, pre, n_ops, True)[0]
            assert b.dtype == raws[n_ops - 1].dtype and torch.equal(_bits(raws[n_ops - 1]), _bits(b)), R.OPS[n_ops - 1].name
        assert torch.equal(m.embed_device(xd, False), m.embed_device(pre, True))
        torch.cuda.synchronize()
        assert lib.alink_resnet50_range_flag(m.h, 0) == 0
    finally:
        restore(lib)


@pytest.mark.parametrize("dt", R.TYPES)
def test_resnet50_nan_stays_in_its_image(gpu, dt):
    """A NaN pixel in image 0 of two: image 1 keeps every bit at every op, and relu_keep_nan / max_keep_nan carry the NaN to image
    0's features (nothing is flushed to zero).  A NaN is ordinary data: nothing faults."""
    size = (197, 228)
    m, lib = _net(size, dt, 2), gpu.load()
    clean = _images(8, 2, size)
    x = clean.clone()
    x[0, 100, 100, 1] = float("nan")
    try:
        if dt == "f16x2":
            _calibrate(gpu, m, clean, True)
        for i, op in enumerate(R.OPS):
            got = _prefix(gpu, m, x, i + 1, True)[0]
            ok = _prefix(gpu, m, clean, i + 1, True)[0]
            assert torch.equal(_bits(got[1]), _bits(ok[1])), "%s: the neighbour image changed" % op.name
            assert torch.isnan(got[0].float()).any(), "%s: the NaN is gone from image 0" % op.name
        assert torch.isnan(got[0]).any() and torch.isfinite(got[1]).all()
    finally:
        torch.cuda.synchronize()
        lib.alink_resnet50_range_flag(m.h, 1)          # the features of image 0 are NaN: the flag went up, as it must
        restore(lib)


def test_resnet50_prefix_refuses_in_words(gpu):
    """workspace too small, n_ops beyond 55, split precision before calibration: -1 and a message, nothing launched"""
    from a_link_amd.resnet50 import VGGResNet50
    fn, lib = _fn(gpu), gpu.load()
    size = (197, 228)
    m = _net(size, "bf16", 2)
    x = _images(1, 1, size)
    ws, wsb = m.ws.get(1)
    need = lib.alink_resnet50_workspace_bytes(m.h, 1)
    st = gpu.current_stream(m.device)
    before = m.ws.tensor().clone()

    def call(h, n_ops, wsb_):
        return fn(h, gpu.ptr(x), 1, 1, None, ws, wsb_, st, n_ops, None, None, None, None, None, 0, None, None, None)
    assert call(m.h, 3, need - 256) == -1 and b"workspace too small" in lib.alink_last_error()
    assert call(m.h, NOPS + 1, wsb) == -1 and b"55 ops" in lib.alink_last_error()
    assert call(m.h, NOPS, wsb) == -1 and b"bad argument" in lib.alink_last_error()      # the whole forward needs dev_out
    assert call(m.h, 0, wsb) == NOPS and call(m.h, -3, wsb) == NOPS
    torch.cuda.synchronize()
    assert torch.equal(m.ws.tensor(), before), "a refused call wrote to the workspace"

    class Uncalibrated(VGGResNet50):
        def calibrate(self, *a, **k):
            pass
    u = Uncalibrated(size, weights=_params(), dtype="f16x2", max_batch=1)
    ws, wsb = u.ws.get(1)
    assert call(u.h, 3, wsb) == -1 and b"calibrate has not run" in lib.alink_last_error()
