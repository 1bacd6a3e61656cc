"""GPU: the few-pixel attack on the SmallRes student (attack.py's pixel scorer).

  1. alink_perturb_resize_multi equals alink_perturb_images_multi(split = 1) + alink_resize_bilinear of each half, bit for bit;
  2. SmallResNet.score_pairs gives a pair the same bits in every batch, and agrees with the torch-CPU oracle;
  3. the lock-step search on the pixel scorer equals the one-pair-after-another search, bit for bit;
  4. noise.AdversarialNoise over a SmallRes student (no feature model), at a source size that is not the model's;
  5. SmallResNet.predict refuses a batch that is not of the model's size;
  6. the Multi-PIE driver runs with --noise adversarial and the three search options.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ---- 1. the fused kernel ---------------------------------------------------------------------------------------------------
def _rows_read(src, dst):
    """source rows (or columns) some destination's two taps read: src_coord of csrc/noise.hip in NumPy"""
    used = set()
    for d in range(dst):
        s = int(np.floor(np.float32((d + 0.5) * (float(src) / float(dst)) - 0.5)))
        s = min(max(s, 0), src - 1)
        used.update((s, min(s + 1, src - 1)))
    return used


def _population(Hc, W, k, seed):
    """15 candidates as the search draws them (the solver's scaled initial population)"""
    from a_link_amd import attack as A
    xs = A.PixelAttacker(None)._solver(0, k, (Hc, W), 3, 15, seed).ask()
    assert xs.shape[1] == 5 * k and xs.shape[0] >= 15
    return np.ascontiguousarray(xs[:15], dtype=np.float64)


def _hand_placed(xs, Hc, W, Ho, Wo):
    """overwrite the first entries of some candidates of search 0 with the edge cases (k >= 3 entries per candidate)"""
    H = Hc // 2

    def put(row, j, r, c, rgb):
        xs[row, 5 * j:5 * j + 5] = (r, c) + tuple(rgb)
    # two entries on one pixel: the last wins
    put(0, 0, 3.7, 4.2, (10.9, 20.1, 30.5))
    put(0, 1, 3.1, 4.9, (200.2, 100.7, 50.0))
    # coordinates at -1, 2H and W: skipped (and -0.5, which truncates to 0: written)
    put(1, 0, -1.0, 5.0, (255.0, 255.0, 255.0))
    put(1, 1, float(Hc), 5.0, (255.0, 255.0, 255.0))
    put(1, 2, 5.0, float(W), (255.0, 255.0, 255.0))
    put(2, 0, 6.0, -1.0, (255.0, 255.0, 255.0))
    put(2, 1, -0.5, -0.5, (1.0, 2.0, 3.0))
    # the seam: the last row of the top half, the first of the bottom half, in one column
    put(3, 0, float(H - 1), 7.0, (255.0, 0.0, 0.0))
    put(3, 1, float(H), 7.0, (0.0, 255.0, 0.0))
    # the four corners of the stacked image
    put(4, 0, 0.0, 0.0, (250.0, 1.0, 1.0))
    put(4, 1, 0.0, float(W - 1), (1.0, 250.0, 1.0))
    put(5, 0, float(Hc - 1), 0.0, (1.0, 1.0, 250.0))
    put(5, 1, float(Hc - 1), float(W - 1), (250.0, 250.0, 1.0))
    # a pixel no tap reads, in either half (where the resize skips source pixels at all)
    free_r = sorted(set(range(H)) - _rows_read(H, Ho))
    free_c = sorted(set(range(W)) - _rows_read(W, Wo))
    if free_r and free_c:
        put(6, 0, float(free_r[0]), float(free_c[0]), (255.0, 255.0, 255.0))
        put(6, 1, float(H + free_r[-1]), float(free_c[-1]), (0.0, 0.0, 0.0))
    return bool(free_r and free_c)


@pytest.mark.parametrize("k", [3, 40])
@pytest.mark.parametrize("Hc,W,Ho,Wo", [(80, 40, 16, 16), (48, 20, 32, 32), (66, 47, 16, 24), (32, 16, 16, 16)])
def test_fused_perturb_resize_equals_the_composition(gpu, Hc, W, Ho, Wo, k):
    import torch
    lib = gpu.load()
    H = Hc // 2
    rng = np.random.RandomState(Hc + W + k)
    imgs = torch.from_numpy((rng.rand(2, Hc, W, 3) * 255).astype(np.float32)).cuda()
    xs_h = np.concatenate([_population(Hc, W, k, 11), _population(Hc, W, k, 12)])
    skipped = _hand_placed(xs_h, Hc, W, Ho, Wo)
    assert skipped == ((Hc, W, Ho, Wo) == (80, 40, 16, 16))
    n, group = 30, 15
    xs = torch.from_numpy(xs_h).cuda()
    of = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    halves = torch.empty((2, n, H, W, 3), dtype=torch.float32, device="cuda")
    gpu.check(lib.alink_perturb_images_multi(gpu.ptr(imgs), gpu.ptr(of), group, gpu.ptr(xs), n, k, Hc, W, 1, gpu.ptr(halves), None))
    want = torch.empty((2, n, Ho, Wo, 3), dtype=torch.float32, device="cuda")
    gpu.check(lib.alink_resize_bilinear(gpu.ptr(halves), gpu.ptr(want), 2 * n, H, W, 3, Ho, Wo, None))
    got = torch.full((2, n, Ho, Wo, 3), -1.0, dtype=torch.float32, device="cuda")
    gpu.check(lib.alink_perturb_resize_multi(gpu.ptr(imgs), gpu.ptr(of), group, gpu.ptr(xs), n, k, Hc, W, Ho, Wo, gpu.ptr(got), None))
    got_h, want_h = got.cpu().numpy(), want.cpu().numpy()
    assert np.array_equal(got_h, want_h), "fused perturb + resize differs from perturb, then resize (%d elements)" % (got_h != want_h).sum()
    if (Ho, Wo) == (H, W):
        assert np.array_equal(got_h, halves.cpu().numpy()), "at the source size the fused kernel is the plain perturb"
    # the perturbation reached the output (the check above is not one of two untouched images)
    base = torch.empty((2, 2, Ho, Wo, 3), dtype=torch.float32, device="cuda")
    gpu.check(lib.alink_resize_bilinear(gpu.ptr(imgs), gpu.ptr(base), 4, H, W, 3, Ho, Wo, None))      # (2 images x 2 halves, image-major)
    b = base.cpu().numpy()
    assert not np.array_equal(got_h[0, 0], b[1, 0]) and (got_h[:, group:] != b[0][:, None]).any()
    # rows of the 30-candidate launch equal the same candidates launched alone
    alone = torch.empty((n, 2, 1, Ho, Wo, 3), dtype=torch.float32, device="cuda")
    for i in range(n):
        gpu.check(lib.alink_perturb_resize_multi(gpu.ptr(imgs), gpu.ptr(of[i // group:]), 1, gpu.ptr(xs[i]), 1, k, Hc, W, Ho, Wo,
                                                 gpu.ptr(alone[i]), None))
    assert np.array_equal(alone.cpu().numpy()[:, :, 0].transpose(1, 0, 2, 3, 4), got_h)


def test_fused_perturb_resize_refuses_what_it_cannot_hold(gpu):
    import torch
    lib = gpu.load()
    img = torch.zeros((1, 8, 4, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 1, 4, 4, 3), dtype=torch.float32, device="cuda")
    xs = torch.zeros((1, 5 * 129), dtype=torch.float64, device="cuda")
    assert lib.alink_perturb_resize_multi(gpu.ptr(img), None, 1, gpu.ptr(xs), 1, 129, 8, 4, 4, 4, gpu.ptr(out), None) != 0      # k > 128
    assert lib.alink_perturb_resize_multi(gpu.ptr(img), None, 1, gpu.ptr(xs), 1, 3, 7, 4, 4, 4, gpu.ptr(out), None) != 0        # odd rows
    gpu.check(lib.alink_perturb_resize_multi(gpu.ptr(img), None, 1, gpu.ptr(xs), 1, 128, 8, 4, 4, 4, gpu.ptr(out), None))         # k = 128 runs


# ---- 2. batch-invariant pair scores ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,feat", [(16, 64), (32, 2048)])
def test_score_pairs_is_batch_invariant(gpu, size, feat):
    import torch
    from a_link_amd.smallres import SmallResNet
    from oracle import smallres as OS
    net = SmallResNet((size, size, 3), feat, lr=0.1, seed=3)
    ws = net.get_weights()
    rng = np.random.RandomState(7)
    for i in range(1, len(ws), 2):                       # non-zero biases
        ws[i] = (rng.randn(*ws[i].shape) * 0.05).astype(np.float32)
    net.set_weights(ws)
    n = 600
    raw_L = rng.randint(0, 256, (n, size, size, 3)).astype(np.float32)
    raw_R = rng.randint(0, 256, (n, size, size, 3)).astype(np.float32)
    Lh, Rh = (raw_L - 128.) / 128., (raw_R - 128.) / 128.
    L, R = torch.from_numpy(Lh).cuda(), torch.from_numpy(Rh).cuda()
    whole_d = net.score_pairs(L, R)
    assert whole_d.is_cuda and tuple(whole_d.shape) == (n, 2)
    whole = whole_d.cpu().numpy()
    np.testing.assert_allclose(whole, OS.SmallResModel(ws).predict([Lh, Rh]), atol=2e-5)
    for m in (1, 2, 255, 256, 257):                      # alone, a small call, around the chunk of 256
        for start in (0, 3, 255, n - m):
            part = net.score_pairs(L[start:start + m], R[start:start + m]).cpu().numpy()
            assert np.array_equal(part, whole[start:start + m]), (size, feat, m, start)
    for i in (1, 256, 511, 512, 599):                    # alone, at and around the chunk boundaries of the whole call
        assert np.array_equal(net.score_pairs(L[i:i + 1], R[i:i + 1]).cpu().numpy(), whole[i:i + 1]), i
    # `out=` is written in place; raw pixels with prescale are the same numbers ((x - 128) / 128 is exact in float32)
    out = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    assert net.score_pairs(torch.from_numpy(raw_L).cuda(), torch.from_numpy(raw_R).cuda(), out=out, prescale=True) is out
    assert np.array_equal(out.cpu().numpy(), whole)
    # the parameters are untouched, and an empty call is one
    for a, b in zip(net.get_weights(), ws):
        assert np.array_equal(a, b)
    assert tuple(net.score_pairs(L[:0], R[:0]).shape) == (0, 2)
    with pytest.raises(ValueError):
        net.score_pairs(L[:, :size - 1], R[:, :size - 1])


# ---- 3 / 4. the search ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def student(gpu):
    """a 16 x 16 SmallRes whose scores are spread enough for some searches to flip a pair"""
    from a_link_amd import siamese
    m = siamese.SmallRes((16, 16, 3), (64,), "student16", 0.1, seed=4)
    ws = m.siamese_net.get_weights()
    ws[14] = ws[14] * np.float32(8.0)
    m.siamese_net.set_weights(ws)
    return m


def test_lockstep_equals_sequential_on_the_pixel_scorer(gpu, student):
    import torch
    from a_link_amd import attack as A, noise as N
    wrapped = N.PredictionWrappedModel(student, None)
    rng = np.random.RandomState(5)
    n = 5
    imgs = [rng.randint(0, 256, (48, 24, 3)).astype(np.float32) for _ in range(n)]
    assert isinstance(A._scorer_for(wrapped, "exact"), A._PixelScorer)
    net = student.siamese_net

    def separate(stacked):
        """score_pairs of stacked pairs through the existing separate calls: halves -> resize_images"""
        st = torch.from_numpy(np.stack(stacked)).cuda()
        l, r = N.resize_images(st[:, :24].contiguous(), (16, 16)), N.resize_images(st[:, 24:].contiguous(), (16, 16))
        return net.score_pairs(l, r, prescale=True).cpu().numpy()
    clean = separate(imgs)
    # pairs 0, 1 ask for the class the clean pair already has, the rest for the other one
    tcs = [int(np.argmax(clean[i])) if i < 2 else 1 - int(np.argmax(clean[i])) for i in range(n)]
    targets = [[1 - t, t] for t in tcs]
    kw = dict(dimensions=(48, 24), pixel_count=3, maxiter=3, popsize=15, seeds=[100 + 7 * i for i in range(n)])
    for early in (True, False):
        seq = A.PixelAttacker(wrapped, lockstep=0)
        want = np.stack(seq.attack_all(imgs, targets, early_stop=early, **kw))
        want_res = seq.last_results
        assert want.shape == (n, 48, 24, 3) and len(want_res) == n
        if not early:
            assert [int(r.nit) for r in want_res] == [3] * n
        for K in (1, 2, 4, 32):
            att = A.PixelAttacker(wrapped, lockstep=K)
            got = att.attack_all(imgs, targets, early_stop=early, **kw)
            assert np.array_equal(np.stack(got), want), (early, K)
            for r, w in zip(att.last_results, want_res):
                assert np.array_equal(r.x, w.x) and r.fun == w.fun and r.nit == w.nit and r.nfev == w.nfev, (early, K)
        # the best member's recorded score row is what the separate calls give for its perturbed, split and resized pair
        rows = separate([A.perturb_image(r.x, im)[0] for r, im in zip(att.last_results, imgs)])
        assert np.array_equal(np.stack([r.scores for r in att.last_results]), rows)
        for r, row, tc in zip(att.last_results, rows, tcs):
            assert r.fun == 1 - row[tc]
    # stacked pairs handed over as ONE device tensor come back as one, the same bits
    dev_out = A.PixelAttacker(wrapped, lockstep=4).attack_all(torch.from_numpy(np.stack(imgs)).cuda(), targets, early_stop=False, **kw)
    assert dev_out.is_cuda and np.array_equal(dev_out.cpu().numpy(), want)


def test_adversarial_noise_over_the_pixel_student(gpu, student):
    import torch
    from a_link_amd import noise as N
    rng = np.random.RandomState(8)
    n, pc = 5, 3
    L = rng.randint(0, 256, (n, 24, 24, 3)).astype(np.float32)
    R = rng.randint(0, 256, (n, 24, 24, 3)).astype(np.float32)
    labels = np.eye(2, dtype=np.float32)[rng.randint(0, 2, n)]
    mk = lambda: N.AdversarialNoise(student, None, None, seed=9, pixel_count=pc, maxiter=2, popsize=15)
    a = mk()
    whole = a.addPairNoise([L, R], labels)
    wl, wr = np.stack(whole[0]), np.stack(whole[1])
    assert wl.shape == L.shape and wr.shape == R.shape
    changed = 0
    for i in range(n):
        dl, dr = (wl[i] != L[i]).any(axis=2), (wr[i] != R[i]).any(axis=2)
        assert dl.sum() + dr.sum() <= pc
        changed += dl.sum() + dr.sum()
        for new, d in ((wl[i], dl), (wr[i], dr)):
            v = new[d]
            assert np.array_equal(v, np.round(v)) and v.min(initial=0) >= 0 and v.max(initial=0) <= 255
    assert changed > 0
    # device tensors in: device tensors out, the same bits
    dev = mk().addPairNoise([torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()], labels)
    assert dev[0].is_cuda and dev[1].is_cuda
    assert np.array_equal(dev[0].cpu().numpy(), wl) and np.array_equal(dev[1].cpu().numpy(), wr)
    # rows=(lo, total) shards reproduce the whole-batch call
    for lo, hi in ((0, 2), (2, 5)):
        part = mk().addPairNoise([L[lo:hi], R[lo:hi]], labels[lo:hi], rows=(lo, n))
        assert np.array_equal(np.stack(part[0]), wl[lo:hi]) and np.array_equal(np.stack(part[1]), wr[lo:hi])
    # an empty shard consumes the stream like any other
    b = mk()
    empty = b.addPairNoise([L[:0], R[:0]], labels[:0], rows=(5, n))
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and b.stream_state() == a.stream_state()

    # a duck-typed model with only `predict` still takes the generic route, and returns
    class OnlyPredict(object):
        calls = 0

        def predict(self, X):
            OnlyPredict.calls += 1
            return np.tile(np.float32([0.5, 0.5]), (len(X[0]), 1))
    out = N.AdversarialNoise(OnlyPredict(), None, None, seed=1, pixel_count=1, maxiter=1, popsize=10).addPairNoise([L[:1], R[:1]], labels[:1])
    assert OnlyPredict.calls > 0 and np.stack(out[0]).shape == (1, 24, 24, 3) and np.stack(out[1]).shape == (1, 24, 24, 3)


# ---- 5. predict's shape check ----------------------------------------------------------------------------------------------
def test_predict_refuses_a_batch_of_another_size(gpu, student):
    net = student.siamese_net
    good = np.zeros((3, 16, 16, 3), np.float32)
    assert net.predict([good, good]).shape == (3, 2)
    for bad in (np.zeros((3, 24, 24, 3), np.float32), np.zeros((3, 12, 12, 3), np.float32), np.zeros((3, 16, 16), np.float32)):
        with pytest.raises(ValueError):
            net.predict([bad, bad])
    with pytest.raises(ValueError):
        net.predict([good, good[:2]])


# ---- 6. the driver ---------------------------------------------------------------------------------------------------------
def _make_mtp(root, n_persons=5, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(root)
    for p in range(1, n_persons + 1):
        for suf in ("01_01_051_06.png", "02_01_051_06.png", "01_01_051_08.png", "02_01_051_08.png", "01_01_130_06.png"):
            Image.fromarray(rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)).save(os.path.join(root, "%03d_%s" % (p, suf)))
    return root


def test_mtp_driver_runs_the_few_pixel_attack(gpu, tmp_path):
    """ALINK_MTP.main end to end on 64 x 64 PNGs with a 32 x 32 student: --noise adversarial and --noise gaussian,adversarial"""
    from a_link_amd import ALINK_MTP
    train, test = _make_mtp(str(tmp_path / "train")), _make_mtp(str(tmp_path / "test"), seed=1)
    models = str(tmp_path / "models")
    os.makedirs(models)

    def args(noises):
        return ["--dataDirPrefix", train, "--testDir", test, "--quiet", "--lowRes", "32", "--noise", noises,
                "--attack_pixels", "3", "--attack_maxiter", "2", "--attack_popsize", "15",
                "--out_model", os.path.join(models, "postALINK"), "--ensemble_basepath", os.path.join(models, "ensemble"),
                "--lowres_basemodel", os.path.join(models, "lowresModel"), "--pretrain_steps", "32", "--lowres_epochs", "1"]
    loop = ["--alink_bs", "2", "--batch_send", "4", "--disparity_ratio", "1.0", "--eps", "0.0", "--ft_epochs", "1", "--active_ratio", "4.0"]
    np.random.seed(0)
    assert ALINK_MTP.main(args("adversarial")) is None                      # first run trains the low-res model and quits
    assert os.path.exists(os.path.join(models, "lowresModel32.h5"))
    for noises in ("adversarial", "gaussian,adversarial"):
        st = ALINK_MTP.main(args(noises) + loop)
        assert os.path.exists(os.path.join(models, "postALINK.h5"))
        assert st.iterations >= 1 and 0.0 <= st.top1 <= 1.0
