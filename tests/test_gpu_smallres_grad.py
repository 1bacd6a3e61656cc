"""GPU: SmallRes input gradients (alink_smallres_input_grad: the dz chain ending in conv1_dgrad_kernel), the adjoint of the
bilinear resize (alink_resize_bilinear_grad) and the FGSM / PGD noise on a pixel student — against torch float64 autograd
through oracle.smallres._tower + the pair head + loss_fn, with the float32 composition of the same on the CPU as the yardstick
of what a float32 implementation can reach."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _imgs(n, s, seed):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n,) + (s if isinstance(s, tuple) else (s, s)) + (3,)).astype(np.float32)


def _net_with_biases(size, feat, seed=3):
    from a_link_amd.smallres import SmallResNet
    net = SmallResNet((size, size, 3), feat, lr=0.1, seed=seed)
    ws = net.get_weights()
    rng = np.random.RandomState(7)
    for i in range(1, len(ws), 2):                       # non-zero biases (as tests/test_gpu_smallres.py)
        ws[i] = (rng.randn(*ws[i].shape) * 0.05).astype(np.float32)
    net.set_weights(ws)
    return net, ws


def _probs(t, L, R):
    from oracle.smallres import _tower
    fl, fr = _tower(t, L), _tower(t, R)
    d = (fl - fr).abs()
    h = F.relu(d @ t[10] + t[11])
    h = F.relu(h @ t[12] + t[13])
    return F.softmax(h @ t[14] + t[15], dim=1)


def _ref_grads(ws, L, R, y, sw, reduction, prescale, dtype, src_to=None):
    """(dL, dR, probs) of the whole call's Keras loss by autograd in `dtype`: inputs -> [resize to src_to] -> [(x - 128) / 128]
    -> tower -> head -> loss_fn ('mean': the sample-weighted batch mean; 'sum': that times count(sw != 0), the plain sum)."""
    from oracle.smallres import loss_fn
    t = [torch.tensor(np.asarray(w), dtype=dtype) for w in ws]
    Lt = torch.tensor(np.asarray(L), dtype=dtype, requires_grad=True)
    Rt = torch.tensor(np.asarray(R), dtype=dtype, requires_grad=True)

    def pre(x):
        if src_to is not None and tuple(x.shape[1:3]) != tuple(src_to):
            x = F.interpolate(x.permute(0, 3, 1, 2), size=src_to, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        return (x - 128.) / 128. if prescale else x
    p = _probs(t, pre(Lt), pre(Rt))
    loss = loss_fn(p, y, sw)
    if reduction == "sum":
        loss = loss * float(len(y) if sw is None else np.count_nonzero(np.asarray(sw)))
    loss.backward()
    return Lt.grad.numpy(), Rt.grad.numpy(), p.detach().numpy()


def _rel_err(g, g64):
    """max |g - g64| / max |g64| per image; images whose float64 gradient is all zero (sample weight 0) must be all zero"""
    n = len(g64)
    d = np.abs(np.asarray(g, np.float64) - g64).reshape(n, -1).max(1)
    m = np.abs(g64).reshape(n, -1).max(1)
    assert np.all(d[m == 0] == 0), "a pair without weight has a non-zero gradient"
    return float((d[m > 0] / m[m > 0]).max())


def _sign_check(g, g64):
    """signs agree wherever |g64| >= 1e-5 of its image's maximum; returns the fraction of elements left out"""
    n = len(g64)
    m = np.abs(g64).reshape(n, -1).max(1).reshape((n,) + (1,) * (g64.ndim - 1))
    big = np.abs(g64) >= 1e-5 * m
    big &= m > 0
    assert np.array_equal(np.sign(np.asarray(g))[big], np.sign(g64)[big]), "sign mismatch on %d elements" % int(
        (np.sign(np.asarray(g))[big] != np.sign(g64)[big]).sum())
    live = np.broadcast_to(m > 0, g64.shape)
    return float((live & ~big).sum()) / max(1, int(live.sum()))


@pytest.mark.parametrize("n", [6, 40])                    # 40: beyond the head's fused path (at most 32 pairs)
@pytest.mark.parametrize("size,feat", [(32, 2048), (48, 256), (16, 64)])
def test_gradient_against_float64_autograd(gpu, size, feat, n):
    """Required: error <= 4 x e32 (the float32 CPU composition's own error against float64, same measure), signs equal wherever
    |g64| >= 1e-5 max|g64| of the image, at most 1e-3 of the elements left out of the sign check."""
    net, ws = _net_with_biases(size, feat)
    rng = np.random.RandomState(11)
    # integer images make exact ties in the 2 x 2 pools likely; a float32 implementation that breaks one the other way has the
    # gradient of ANOTHER pool winner (errors of 1e-3 and more).  The input seed is one at which the float32 yardstick itself is
    # tie-free (asserted below: e32 near the format's precision), chosen on the CPU references alone.
    seed = 101 if (size, n) == (32, 40) else 1
    raw = [_imgs(n, size, seed), _imgs(n, size, seed + 1)]
    y = np.eye(2, dtype=np.float32)[rng.randint(0, 2, n)]
    sw_full = np.resize(np.array([1, 0.5, 0, 2, 1, 1], np.float32), n)
    for prescale in (True, False):
        x = raw if prescale else [(r - 128.) / 128. for r in raw]
        for sw in (None, sw_full):
            for reduction in ("mean", "sum"):
                g64 = _ref_grads(ws, x[0], x[1], y, sw, reduction, prescale, torch.float64)
                g32 = _ref_grads(ws, x[0], x[1], y, sw, reduction, prescale, torch.float32)
                got = net.input_gradients(x, y, sample_weight=sw, reduction=reduction, prescale=prescale)
                assert all(g.is_cuda and g.dtype is torch.float32 and tuple(g.shape) == x[0].shape for g in got)
                got = [g.cpu().numpy() for g in got]
                e32 = max(_rel_err(g32[0], g64[0]), _rel_err(g32[1], g64[1]))
                err = max(_rel_err(got[0], g64[0]), _rel_err(got[1], g64[1]))
                out32 = max(_sign_check(g32[0], g64[0]), _sign_check(g32[1], g64[1]))
                out = max(_sign_check(got[0], g64[0]), _sign_check(got[1], g64[1]))
                print("size %d feat %d n %d prescale %d sw %d %s: e32 %.3g kernels %.3g ratio %.2f; left out of the sign check %.2g (f32 %.2g)"
                      % (size, feat, n, prescale, sw is not None, reduction, e32, err, err / e32, out, out32))
                assert e32 < 1e-5, "the float32 yardstick itself flipped a tie at this input seed: %g" % e32
                assert err <= 4 * e32, (err, e32)
                assert out <= 1e-3, out


def test_device_operands_and_shape_guard(gpu):
    net, _ = _net_with_biases(16, 64)
    L, R = _imgs(4, 16, 3), _imgs(4, 16, 4)
    y = np.eye(2, dtype=np.float32)[[0, 1, 1, 0]]
    a = net.input_gradients([L, R], y, prescale=True)
    b = net.input_gradients([torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()], torch.from_numpy(y).cuda(), prescale=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        net.input_gradients([_imgs(4, 32, 3), _imgs(4, 32, 4)], y)
    with pytest.raises(ValueError):
        net.input_gradients([L, R], y, reduction="max")


def test_nothing_else_moves(gpu):
    """input_gradients leaves weights and predict bit-equal, and a following train_on_batch (explicit masks) leaves the weights
    bit-equal to those of a twin that never called it."""
    net, ws = _net_with_biases(32, 256)
    twin, _ = _net_with_biases(32, 256)
    rng = np.random.RandomState(5)
    n = 6
    L, R = (_imgs(n, 32, 1) - 128.) / 128., (_imgs(n, 32, 2) - 128.) / 128.
    y = np.eye(2, dtype=np.float32)[rng.randint(0, 2, n)]
    before = net.predict([L, R])
    net.input_gradients([L, R], y, reduction="sum")
    net.input_gradients([L, R], y, sample_weight=np.array([1, 0.5, 0, 2, 1, 1], np.float32))
    for a, b in zip(net.get_weights(), ws):
        assert np.array_equal(a, b)
    assert np.array_equal(net.predict([L, R]), before)
    masks = (rng.rand(2 * n * sum(net.mask_sizes)) >= 0.25).astype(np.uint8)
    m1 = net.train_on_batch([L, R], y, masks=masks)
    m2 = twin.train_on_batch([L, R], y, masks=masks)
    assert m1 == m2
    for a, b in zip(net.get_weights(), twin.get_weights()):
        assert np.array_equal(a, b)


def test_chunking(gpu):
    """300 pairs, reduction='sum': rows 0:256 and 256:300 are bit-equal to calls on those rows alone"""
    net, _ = _net_with_biases(16, 64)
    n = 300
    L, R = _imgs(n, 16, 1), _imgs(n, 16, 2)
    y = np.eye(2, dtype=np.float32)[np.random.RandomState(3).randint(0, 2, n)]
    whole = net.input_gradients([L, R], y, reduction="sum", prescale=True)
    for lo, hi in ((0, 256), (256, 300)):
        part = net.input_gradients([L[lo:hi], R[lo:hi]], y[lo:hi], reduction="sum", prescale=True)
        assert torch.equal(whole[0][lo:hi], part[0]) and torch.equal(whole[1][lo:hi], part[1])
    # 'mean' is the mean over ALL rows whatever the chunking: the same gradients scaled by 1/300
    mean = net.input_gradients([L, R], y, prescale=True)
    w0 = whole[0].cpu().numpy()
    np.testing.assert_allclose(mean[0].cpu().numpy() * 300, w0, rtol=0, atol=1e-5 * np.abs(w0).max())


@pytest.mark.parametrize("src,dst", [((64, 64), (32, 32)), ((40, 40), (16, 16)), ((32, 32), (48, 48)), ((50, 70), (32, 32))])
def test_resize_adjoint(gpu, src, dst):
    from a_link_amd import noise
    n = 5
    x = _imgs(n, src, 9)
    dout = np.random.RandomState(4).randn(n, dst[0], dst[1], 3).astype(np.float32)

    def autograd(dtype):
        xt = torch.tensor(x, dtype=dtype, requires_grad=True)
        out = F.interpolate(xt.permute(0, 3, 1, 2), size=dst, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        out.backward(torch.tensor(dout, dtype=dtype))
        return out.detach().numpy(), xt.grad.numpy()
    f64, g64 = autograd(torch.float64)
    _, g32 = autograd(torch.float32)
    fwd = noise.resize_images(x, (dst[1], dst[0]))
    # the reference IS the forward's rule.  The kernel keeps a tap weight in float32 after taking it from a coordinate below 128
    # (spacing 2^-17): half a spacing per axis on pixel differences of up to 255 is 2 x 3.8e-6 x 255 = 1.9e-3, plus the
    # arithmetic's own 1e-4; another rule (corner-aligned, nearest) is off by tens of grey levels
    np.testing.assert_allclose(fwd, f64, rtol=0, atol=2.5e-3)
    got_t = noise.resize_images_grad(torch.from_numpy(dout).cuda(), (src[1], src[0]))
    again = noise.resize_images_grad(torch.from_numpy(dout).cuda(), (src[1], src[0]))
    assert got_t.is_cuda and tuple(got_t.shape) == x.shape and torch.equal(got_t, again)
    got = noise.resize_images_grad(dout, (src[1], src[0]))
    assert isinstance(got, np.ndarray) and np.array_equal(got, got_t.cpu().numpy())
    e32, err = _rel_err(g32, g64), _rel_err(got, g64)
    zeros = float((g64 == 0).mean())
    print("resize adjoint %s -> %s: e32 %.3g kernel %.3g; %.1f %% of the source elements untouched" % (src, dst, e32, err, 100 * zeros))
    assert err <= 4 * e32, (err, e32)
    assert np.all(got[g64 == 0] == 0.0)
    # <Rx, dout> = <x, R^T dout>: the adjoint identity against the forward kernel itself
    lhs, rhs = float((fwd.astype(np.float64) * dout).sum()), float((x.astype(np.float64) * got).sum())
    assert abs(lhs - rhs) <= 1e-5 * np.abs(fwd.astype(np.float64) * dout).sum()


def test_resize_adjoint_identity(gpu):
    from a_link_amd import noise
    g = np.random.RandomState(1).randn(3, 24, 20, 3).astype(np.float32)
    assert np.array_equal(noise.resize_images_grad(g, (20, 24)), g)
    gt = torch.from_numpy(g).cuda()
    out = noise.resize_images_grad(gt, (20, 24))
    assert torch.equal(out, gt) and out.data_ptr() != gt.data_ptr()


def _student(tmp_path, seed=1):
    from a_link_amd import siamese
    return siamese.SmallRes((32, 32, 3), (2048,), str(tmp_path / "student"), 0.1, seed=seed)


def _target_prob(p, y):
    return (np.asarray(p, np.float64) * y).sum(1)


@pytest.mark.parametrize("pair_size", [32, 64])
def test_attack_on_a_pixel_student(gpu, tmp_path, pair_size):
    from a_link_amd import noise
    m = _student(tmp_path)
    ws = m.siamese_net.get_weights()
    n, eps = 8, 4.0
    L, R = _imgs(n, pair_size, 21), _imgs(n, pair_size, 22)
    y = np.eye(2, dtype=np.float32)[np.random.RandomState(6).randint(0, 2, n)]
    gL, gR, p0 = _ref_grads(ws, L, R, y, None, "sum", True, torch.float64, src_to=(32, 32))
    want = [np.clip(x - eps * np.sign(g), 0, 255) for x, g in ((L, gL), (R, gR))]
    # precondition, on the float64 oracle: the step built from its gradient raises the target-class probability of every pair
    _, _, p1 = _ref_grads(ws, want[0], want[1], y, None, "sum", True, torch.float64, src_to=(32, 32))
    gain = _target_prob(p1, y) - _target_prob(p0, y)
    print("oracle gain of the target-class probability per pair (FGSM, %d x %d pairs): min %.4f max %.4f" % (pair_size, pair_size, gain.min(), gain.max()))
    assert np.all(gain > 0), gain

    def student_probs(pair):
        return m.predict([noise.resize_images(pair[0], (32, 32)), noise.resize_images(pair[1], (32, 32))])
    base = _target_prob(student_probs([L, R]), y)
    np.testing.assert_allclose(base, _target_prob(p0, y), atol=2e-5)
    for name, att in (("fgsm", noise.FGSM(model=m, feature_model=None, eps=eps)),
                      ("pgd", noise.PGD(model=m, feature_model=None, eps=eps, alpha=2.0, steps=3, seed=5))):
        out = att.addPairNoise([L, R], y)
        assert all(isinstance(o, np.ndarray) and o.shape == L.shape and o.dtype == np.float32 for o in out)
        for o, x in zip(out, (L, R)):
            assert np.abs(o - x).max() <= eps and o.min() >= 0 and o.max() <= 255
        rise = _target_prob(student_probs(out), y) - base
        print("%s: rise of the student's target-class probability per pair: min %.4f max %.4f" % (name, rise.min(), rise.max()))
        assert np.all(rise > 0), (name, rise)
        if name == "fgsm":
            off = max(float((o != w).mean()) for o, w in zip(out, want))
            print("fgsm: elements differing from clip(x - eps sign(g64)): %.2g" % off)
            assert off <= 1e-3, off
    # a device tensor in gives a device tensor out, equal to the host form
    att = noise.FGSM(model=m, feature_model=None, eps=eps)
    host = att.addPairNoise([L, R], y)
    dev = att.addPairNoise([torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()], y)
    assert all(isinstance(d, torch.Tensor) and d.is_cuda for d in dev)
    assert all(np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev, host))
    # class labels instead of one-hot targets
    lab = att.addPairNoise([L, R], y.argmax(1))
    assert all(np.array_equal(a, b) for a, b in zip(lab, host))


def test_attack_row_ranges_and_guard(gpu, tmp_path):
    from a_link_amd import noise
    m = _student(tmp_path)
    n = 6
    L, R = _imgs(n, 64, 31), _imgs(n, 64, 32)
    y = np.eye(2, dtype=np.float32)[np.random.RandomState(8).randint(0, 2, n)]
    mk = lambda: noise.PGD(model=m, feature_model=None, eps=4.0, alpha=2.0, steps=1, random_start=True, seed=17)
    whole = mk().addPairNoise([L, R], y)
    a = mk()
    part = a.addPairNoise([L[2:6], R[2:6]], y[2:6], rows=(2, 6))
    for w, p in zip(whole, part):
        assert float((w[2:6] != p).mean()) <= 1e-3
    # an empty shard consumes the call's streams like any other
    b = mk()
    empty = b.addPairNoise([L[:0], R[:0]], y[:0], rows=(6, 6))
    assert len(empty[0]) == 0 and b.stream_state() == a.stream_state()

    class Neither(object):
        def predict(self, X):
            return np.zeros((len(X[0]), 2), np.float32)
    with pytest.raises(TypeError):
        noise.FGSM(model=Neither(), feature_model=None).addPairNoise([L, R], y)
    with pytest.raises(TypeError):
        noise.PGD(model=m, feature_model=None).addNoise(L, y)


def _make_mtp(root, n_persons=5, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(root)
    for p in range(1, n_persons + 1):
        for suf in ("01_01_051_06.png", "02_01_051_06.png", "01_01_051_08.png", "02_01_051_08.png", "01_01_130_06.png"):
            Image.fromarray(rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)).save(os.path.join(root, "%03d_%s" % (p, suf)))
    return root


def test_mtp_driver_runs_gradient_noise(gpu, tmp_path):
    """ALINK_MTP.main end to end on 64 x 64 PNGs with a 32 x 32 student: --noise gaussian,fgsm and --noise pgd"""
    from a_link_amd import ALINK_MTP
    train, test = _make_mtp(str(tmp_path / "train")), _make_mtp(str(tmp_path / "test"), seed=1)
    models = str(tmp_path / "models")
    os.makedirs(models)

    def args(noises):
        return ["--dataDirPrefix", train, "--testDir", test, "--quiet", "--lowRes", "32", "--noise", noises,
                "--out_model", os.path.join(models, "postALINK"), "--ensemble_basepath", os.path.join(models, "ensemble"),
                "--lowres_basemodel", os.path.join(models, "lowresModel"), "--pretrain_steps", "32", "--lowres_epochs", "1"]
    loop = ["--alink_bs", "2", "--batch_send", "4", "--disparity_ratio", "1.0", "--eps", "0.0", "--ft_epochs", "1", "--active_ratio", "4.0"]
    np.random.seed(0)
    assert ALINK_MTP.main(args("gaussian,fgsm")) is None                    # first run trains the low-res model and quits
    assert os.path.exists(os.path.join(models, "lowresModel32.h5"))
    for noises in ("gaussian,fgsm", "pgd"):
        st = ALINK_MTP.main(args(noises) + loop)
        assert os.path.exists(os.path.join(models, "postALINK.h5"))
        assert st.iterations >= 1 and 0.0 <= st.top1 <= 1.0
