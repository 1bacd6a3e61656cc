"""GPU: the input-gradient pass of the VGGFace2 ResNet-50 (csrc/resnet50.hip from alink_resnet50_input_grad on,
csrc/resnet50_bwd.hip) against float64 autograd through a differentiable restatement of oracle/vgg_resnet50.forward
(which runs under no_grad), and the FGSM / PGD noise and the driver flags that reach it.

The tolerance of the gradient test is not a constant.  The error of a 16-bit gradient pass is dominated by ReLU masks that
flip when the forward's activations are stored in 16 bits; the reference alone shows how large that is: the same float64
autograd with every stored activation (stem output, the two inner activations of each unit, the projection, the unit
output) rounded to the mode's type in the forward, straight through.  Per image that gives E_rel and E_(1-cos); the GPU —
which rounds its sums in another order and so flips a different, equally large set of masks — must stay within
1.5 x E_rel and 2.25 x E_(1-cos) (1 - cos ~ rel^2 / 2).  That the bound still tells a structural mistake from rounding is
checked on the CPU: dropping the shortcut or the residual branch of conv2_2 / conv3_1 / conv4_4 / conv5_3 from the
reference gradient must move it by more than the bound.

Measured on MI355X, per image (the three images of the `ref` fixture):
  bf16  rel 0.242 / 0.244 / 0.245 (bounds 0.321 / 0.335 / 0.322), 1 - cos 2.92e-2 / 2.97e-2 / 3.00e-2 (bounds 5.1e-2 / 5.6e-2 / 5.2e-2)
  f16   rel 0.0867 / 0.0872 / 0.0888 (bounds 0.125 / 0.106 / 0.119), 1 - cos 3.75e-3 / 3.80e-3 / 3.94e-3 (bounds 7.8e-3 / 5.7e-3 / 7.1e-3)
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

UNITS = (3, 4, 6, 3)
MEAN_BGR = (91.4953, 103.8827, 131.0912)
BN_EPS = 1e-3
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
DROPPED = ("conv2_2", "conv3_1", "conv4_4", "conv5_3")


def _forward64(params, x_raw, round_to=None, detach=None):
    """oracle.vgg_resnet50.forward restated as a differentiable float64 function of RAW RGB pixels (N, H, W, 3).
    round_to: a torch dtype — every stored activation is rounded to it in the forward, straight through in the backward.
    detach: (unit, "shortcut" | "branch") — that path of that unit carries no gradient."""
    t = lambda n: torch.from_numpy(np.ascontiguousarray(params[n])).double()
    q = (lambda v: v) if round_to is None else (lambda v: v + (v.to(round_to).double() - v).detach())

    def conv_bn(x, name, stride=1, pad=0, relu=True):
        w = t(name + "/kernel").permute(3, 2, 0, 1).contiguous()
        x = F.conv2d(x, w, stride=stride, padding=pad)
        g, b, mu, var = (t(name + "/bn/" + s) for s in ("gamma", "beta", "moving_mean", "moving_variance"))
        x = (x - mu[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + BN_EPS) * g[None, :, None, None] \
            + b[None, :, None, None]
        return F.relu(x) if relu else x
    # preprocess_input(version=2) subtracts the means in float32 (so does the stem kernel's loader): the same numbers here, as a
    # constant offset (derivative 1) that is exact in float64 for 8-bit pixels
    flipped = x_raw.detach().float().flip(-1)
    offset = (flipped - torch.tensor(MEAN_BGR, dtype=torch.float32)).double() - flipped.double()
    x = x_raw.flip(-1) + offset
    x = x.permute(0, 3, 1, 2)
    H, W = x.shape[2], x.shape[3]
    th = max((-(-H // 2) - 1) * 2 + 7 - H, 0)
    tw = max((-(-W // 2) - 1) * 2 + 7 - W, 0)
    x = F.pad(x, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
    x = q(conv_bn(x, "conv1/7x7_s2", stride=2))
    x = F.max_pool2d(x, 3, 2)
    for s in range(4):
        for u in range(1, UNITS[s] + 1):
            p = "conv%d_%d_" % (s + 2, u)
            st = 2 if (u == 1 and s > 0) else 1
            y = q(conv_bn(x, p + "1x1_reduce", stride=st))
            y = q(conv_bn(y, p + "3x3", pad=1))
            y = conv_bn(y, p + "1x1_increase", relu=False)
            sc = q(conv_bn(x, p + "1x1_proj", stride=st, relu=False)) if u == 1 else x
            if detach is not None and detach[0] == p[:-1]:
                if detach[1] == "shortcut":
                    sc = sc.detach()
                else:
                    y = y.detach()
            x = q(F.relu(y + sc))
    x = F.avg_pool2d(x, 7)
    return x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)


def _grad64(params, x, dfeat, **kw):
    xr = torch.from_numpy(x).double().requires_grad_(True)
    f = _forward64(params, xr, **kw)
    (f * torch.from_numpy(dfeat).double()).sum().backward()
    return f.detach().numpy(), xr.grad.numpy()


def _rel_cos(g, ref):
    a, b = np.asarray(g, np.float64).reshape(len(g), -1), np.asarray(ref, np.float64).reshape(len(ref), -1)
    rel = np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    cos = (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return rel, 1.0 - cos


@pytest.fixture(scope="module")
def ref():
    """inputs, the float64 reference gradient, the reference's own 16-bit error E per mode, and the one-path-dropped gradients"""
    from a_link_amd import resnet50 as R
    from oracle import vgg_resnet50 as O
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    params = R.synthetic_params(1)
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (3, 224, 224, 3)).astype(np.float32)
    dfeat = rng.standard_normal((3, 2048)).astype(np.float32)
    feat, g_ref = _grad64(params, x, dfeat)
    want = O.forward(params, O.preprocess_input_v2(x), dtype=torch.float64)
    diff = np.abs(feat - want).max()
    print("restatement against oracle.vgg_resnet50.forward in float64: max |d| %.3g (features up to %.3g)" % (diff, np.abs(want).max()))
    assert diff <= 5e-12, "the differentiable restatement is not the oracle's forward"
    E = {}
    for mode, dt in TORCH_DT.items():
        _, g_q = _grad64(params, x, dfeat, round_to=dt)
        E[mode] = _rel_cos(g_q, g_ref)
        print("%s: reference with 16-bit stored activations: E_rel %s  E_(1-cos) %s" % (mode, E[mode][0], E[mode][1]))
    dropped = {}
    for unit in DROPPED:
        for path in ("shortcut", "branch"):
            _, g_d = _grad64(params, x, dfeat, detach=(unit, path))
            dropped[(unit, path)] = _rel_cos(g_d, g_ref)[0]
            print("reference without the %s of %s: rel %s" % (path, unit, dropped[(unit, path)]))
    return dict(params=params, x=x, dfeat=dfeat, g_ref=g_ref, E=E, dropped=dropped)


def _net(params, dtype, max_batch=4, **kw):
    from a_link_amd.resnet50 import VGGResNet50
    return VGGResNet50(image_size=(224, 224), weights=params, dtype=dtype, max_batch=max_batch, enable_grad=True, **kw)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_input_gradient_matches_autograd(gpu, ref, dtype):
    E_rel, E_cos = ref["E"][dtype]
    bound_rel, bound_cos = 1.5 * E_rel, 2.25 * E_cos
    # the bound must tell a structural mistake from rounding: every dropped path moves the reference by more than it
    for key, rel_d in ref["dropped"].items():
        assert (rel_d > bound_rel).all(), "dropping the %s of %s moves the gradient by %s, inside the bound %s" % (key[1], key[0], rel_d, bound_rel)
    net = _net(ref["params"], dtype)
    xd = torch.from_numpy(ref["x"]).cuda()
    dfd = torch.from_numpy(ref["dfeat"]).cuda()
    feat = net.embed_with_cache(xd)
    assert torch.equal(feat, net.embed_device(xd)), "the cached forward is not the plain forward bit for bit"
    g = net.input_gradient(dfd).cpu().numpy()
    assert g.shape == ref["x"].shape and np.isfinite(g).all()
    rel, omc = _rel_cos(g, ref["g_ref"])
    msg = "%s: GPU rel %s (bound %s = 1.5 x E_rel %s); 1 - cos %s (bound %s = 2.25 x E %s)" % (dtype, rel, bound_rel, E_rel, omc, bound_cos, E_cos)
    print(msg)
    assert (rel <= bound_rel).all() and (omc <= bound_cos).all(), msg
    # preprocessed input (BGR, mean-subtracted): the same features, and the raw-pixel gradient with its channels reversed
    from oracle import vgg_resnet50 as O
    xp = torch.from_numpy(O.preprocess_input_v2(ref["x"])).cuda()
    fp = net.embed_with_cache(xp, preprocessed=True)
    assert torch.equal(fp, net.embed_device(xp, preprocessed=True))
    gp = net.input_gradient(dfd).cpu().numpy()
    # (RESNET50.preprocess subtracts the same float32 means the stem's loader does: the network sees the same numbers)
    assert torch.equal(fp, feat)
    assert np.array_equal(gp[..., ::-1], g)


def test_linearity_and_range(gpu, ref):
    """Masks are fixed by the cache, so input_gradient is linear in dfeat up to the rounding of the stored gradients."""
    E_rel, _ = ref["E"]["f16"]
    net = _net(ref["params"], "f16")
    net.embed_with_cache(torch.from_numpy(ref["x"]).cuda())
    a = torch.from_numpy(ref["dfeat"]).cuda()
    ga = net.input_gradient(a)
    # range: gradients 2^-20 times smaller (|dfeat| / 49 ~ 2e-8: below float16's subnormals) come out 2^-20 times smaller
    small = net.input_gradient(a * 2.0 ** -20) * 2.0 ** 20
    assert float(small.abs().max()) > 0
    rel, _ = _rel_cos(small.cpu().numpy(), ga.cpu().numpy())
    print("scaled by 2^-20 and back: rel %s" % rel)
    assert (rel <= 1.5 * E_rel).all(), rel
    # the per-call scale is a power of two from max|dfeat|: the two calls compute on the same 16-bit values
    assert torch.equal(small, ga)
    # additivity.  A gradient crosses 50 stored 16-bit tensors on its way (the pooled map, three per unit, the stem map), each
    # rounded to float16's unit roundoff u = 2^-11; three evaluations, errors adding linearly at worst: 3 x 50 x 2^-11 = 0.073
    rng = np.random.default_rng(5)
    b = torch.from_numpy(rng.standard_normal((3, 2048)).astype(np.float32)).cuda()
    gb, gab = net.input_gradient(b), net.input_gradient(a + b)
    rel, _ = _rel_cos((ga + gb).cpu().numpy(), gab.cpu().numpy())
    print("additivity: rel %s" % rel)
    assert (rel <= 3 * 50 * 2.0 ** -11).all(), rel


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_deterministic_and_batch_limit(gpu, ref, dtype):
    net = _net(ref["params"], dtype)
    xd = torch.from_numpy(ref["x"]).cuda()
    dfd = torch.from_numpy(ref["dfeat"]).cuda()
    f1 = net.embed_with_cache(xd)
    g1 = net.input_gradient(dfd)
    g2 = net.input_gradient(dfd)
    f3 = net.embed_with_cache(xd)
    g3 = net.input_gradient(dfd)
    assert torch.equal(g1, g2) and torch.equal(g1, g3) and torch.equal(f1, f3)
    with pytest.raises(AssertionError):                      # as IRBackbone: one call takes at most max_batch images
        net.embed_with_cache(torch.zeros((5, 224, 224, 3), device="cuda"))


def test_guards(gpu, ref):
    from a_link_amd import _abi, noise as N, siamese
    from a_link_amd.resnet50 import VGGResNet50
    plain = VGGResNet50(image_size=(224, 224), weights=ref["params"], dtype="bf16", max_batch=2)
    assert not plain.grad_enabled
    with pytest.raises(_abi.AlinkError):
        plain.embed_with_cache(torch.zeros((1, 224, 224, 3), device="cuda"))
    with pytest.raises(_abi.AlinkError):
        VGGResNet50(image_size=(224, 224), weights=ref["params"], dtype="f16x2", max_batch=2, enable_grad=True)
    # without enable_grad nothing more is allocated: the workspace is the forward's, the gradient workspace does not exist
    assert plain.lib.alink_resnet50_grad_workspace_bytes(plain.h, 2) == 0
    fm = siamese.RESNET50((224, 224), weights=ref["params"], dtype="bf16", max_batch=2)
    assert not hasattr(fm, "grad_backbone")
    pm = siamese.SiameseNetwork((2048,), "m2", 0.1, seed=4)
    x = ref["x"][:2]
    with pytest.raises(TypeError):
        N.FGSM(model=pm, feature_model=fm).addPairNoise([x, x[::-1].copy()], np.array([0, 1]))


@pytest.mark.parametrize("grad_dtype", ["bf16", "f16"])
def test_fgsm_and_pgd_through_resnet50(gpu, ref, grad_dtype):
    from a_link_amd import noise as N, siamese
    fm = siamese.RESNET50((224, 224), weights=ref["params"], max_batch=4, grad_dtype=grad_dtype)
    bb = fm.grad_backbone
    assert bb.grad_enabled and bb.dtype == grad_dtype and fm.model.dtype == "f16x2" and not fm.model.grad_enabled
    pm = siamese.SiameseNetwork((2048,), "m2", 0.1, seed=4)
    rng = np.random.RandomState(0)
    n, eps = 6, 6.0
    L = rng.randint(0, 256, (n, 224, 224, 3)).astype(np.float32)
    R = rng.randint(0, 256, (n, 224, 224, 3)).astype(np.float32)
    target = rng.randint(0, 2, n)
    # every existing result stays the exact mode's
    clean = fm.process(L)
    assert np.array_equal(clean, siamese.RESNET50((224, 224), weights=ref["params"], max_batch=4).process(L))
    before = pm.predict([clean, fm.process(R)])[np.arange(n), target]
    for cls, kw in ((N.FGSM, dict(eps=eps)), (N.PGD, dict(eps=eps, alpha=2.0, steps=3, seed=1))):
        att = N.get_relevant_noise(cls.__name__.lower())(model=pm, sess=None, feature_model=fm, **kw)
        al, ar = att.addPairNoise([L, R], target)
        assert al.shape == L.shape and ar.shape == R.shape
        assert np.abs(al - L).max() <= eps + 1e-4 and np.abs(ar - R).max() <= eps + 1e-4
        assert al.min() >= 0 and al.max() <= 255 and ar.min() >= 0 and ar.max() <= 255
        assert np.abs(al - L).max() > 0 and np.abs(ar - R).max() > 0
        after = pm.predict([fm.process(al), fm.process(ar)])[np.arange(n), target]
        # whether the score moves is a property of the random scorer: reported, not gated
        print("%s through RESNET50(grad_dtype=%s): target-class score up on %d of %d pairs, mean %.6f -> %.6f"
              % (cls.__name__, grad_dtype, int((after > before).sum()), n, before.mean(), after.mean()))
        if cls is N.FGSM:
            # one targeted step = clip(x - eps sign(g)) with g from input_gradient itself, in the attack's own order and chunks
            head = pm.siamese_net
            y = torch.from_numpy(att._targets(target, n, head.out_dim)).cuda()
            want_l, want_r = np.empty_like(L), np.empty_like(R)
            for s in range(0, n, bb.max_batch):
                sl = slice(s, min(n, s + bb.max_batch))
                xl, xr = torch.from_numpy(L[sl]).cuda(), torch.from_numpy(R[sl]).cuda()
                er = bb.embed_device(xr)
                el = bb.embed_with_cache(xl)
                dL, _ = head.input_gradients(el, er, y[sl])
                gl = bb.input_gradient(dL).cpu().numpy()
                er = bb.embed_with_cache(xr)
                _, dR = head.input_gradients(el, er, y[sl])
                gr = bb.input_gradient(dR).cpu().numpy()
                assert np.abs(gl).max() > 0 and np.abs(gr).max() > 0
                want_l[sl] = np.clip(L[sl] - np.float32(eps) * np.sign(gl), 0, 255)
                want_r[sl] = np.clip(R[sl] - np.float32(eps) * np.sign(gr), 0, 255)
            assert np.array_equal(al, want_l) and np.array_equal(ar, want_r)


def _make_dfw(root, n_persons=6, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    d = os.path.join(root, "Training_data")
    for p in range(n_persons):
        pd = os.path.join(d, "person%02d" % p)
        os.makedirs(pd)
        for name, size in (("%02d.png" % p, (130, 120)), ("%02d_a.png" % p, (112, 112)), ("%02d_h_001.png" % p, (90, 100)),
                           ("%02d_h_002.png" % p, (150, 140)), ("%02d_I_001.png" % p, (112, 112))):
            Image.fromarray(rng.randint(0, 256, size + (3,)).astype(np.uint8)).save(os.path.join(pd, name))
    return root


@pytest.mark.parametrize("feature_model,noises", [("resnet50", "gaussian,fgsm"), ("arcface", "pgd")])
def test_driver_runs_gradient_noise(gpu, tmp_path, feature_model, noises):
    from a_link_amd import ALINK_arc
    root = _make_dfw(str(tmp_path))
    models = str(tmp_path / "models")
    os.makedirs(models)
    common = ["--dataDirPrefix", root, "--arcface_model", "synthetic:r18:2", "--feature_model", feature_model, "--quiet",
              "--out_model", os.path.join(models, "postALINK"), "--ensemble_basepath", os.path.join(models, "ensemble"),
              "--disguised_basemodel", os.path.join(models, "disguisedModel"), "--pretrain_steps", "64",
              "--dig_epochs", "1", "--undig_epochs", "1", "--noise", noises]
    np.random.seed(0)
    assert ALINK_arc.main(common + ["--train_disguised_model"]) is None
    st = ALINK_arc.main(common + ["--alink_bs", "3", "--batch_send", "8", "--disparity_ratio", "0.9", "--eps", "0.0001",
                                  "--ft_epochs", "1"])
    assert os.path.exists(os.path.join(models, "postALINK.h5"))
    assert st.iterations >= 1 and st.un_size > 0 and st.active_count >= 0
