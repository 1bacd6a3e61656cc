"""GPU: SmallRes gallery identification — every face embedded once, the pair head on the P x G feature pairs, each probe's
argmax / rank on the device.
  1. SmallResNet.features gives an image the same bits alone, in any batch and across the 512-image chunk;
  2. SmallResNet.score_matrix on those features equals score_pairs (existing code: the yardstick) on the materialised pixel
     pairs bit for bit, for tiles that straddle probe rows and every `col`;
  3. alink_identify_rows against NumPy (argmax of the flattened row, stable argsort) on synthetic scores with ties;
  4. siamese.SmallRes.identify equals a literal one-probe-per-call loop on score_pairs, whatever the chunking;
  5. none of it touches the weights or predict's bits;
  6. ALINK_MTP.main --gallery_eval on the synthetic Multi-PIE tree.
All comparisons are exact."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 31, 32, 33, 65)          # around the head kernel's tile of 32 pairs


def _net(size, feat, seed=3):
    from a_link_amd.smallres import SmallResNet
    net = SmallResNet((size, size, 3), feat, lr=0.1, seed=seed)
    ws = net.get_weights()
    rng = np.random.RandomState(7)
    for i in range(1, len(ws), 2):                       # non-zero biases
        ws[i] = (rng.randn(*ws[i].shape) * 0.05).astype(np.float32)
    ws[14] = ws[14] * np.float32(8.0)                    # scores spread away from 0.5
    net.set_weights(ws)
    return net


# ---- 1. features ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,feat", [(16, 64), (32, 2048)])
def test_features_are_batch_invariant(gpu, size, feat):
    import torch
    net = _net(size, feat)
    n = 515                                              # crosses the chunk of 512 images
    raw = torch.from_numpy(np.random.RandomState(1).randint(0, 256, (n, size, size, 3)).astype(np.float32)).cuda()
    whole = net.features(raw, prescale=True)
    assert whole.is_cuda and whole.dtype is torch.float32 and tuple(whole.shape) == (n, feat)
    assert float(whole.min()) >= 0.0 and float(whole.max()) > 0.0                          # a ReLU's output, not all dead
    for k in (0, 1, 511, 512, n - 1):                    # alone (n = 1): first, around the chunk boundary, last
        assert torch.equal(net.features(raw[k:k + 1], prescale=True)[0], whole[k]), (size, feat, k)
    assert torch.equal(net.features(raw[500:], prescale=True), whole[500:])               # a small batch at another offset
    # prescale is (x - 128) / 128, exact in float32; `out=` is written in place; host arrays are taken too
    out = torch.empty((n, feat), dtype=torch.float32, device="cuda")
    assert net.features((raw - 128.) / 128., out=out, prescale=False) is out and torch.equal(out, whole)
    assert torch.equal(net.features(raw[:4].cpu().numpy(), prescale=True), whole[:4])
    assert tuple(net.features(raw[:0]).shape) == (0, feat)
    with pytest.raises(ValueError):
        net.features(raw[:, :size - 1])
    with pytest.raises(ValueError):
        net.features(raw, out=torch.empty((n, feat + 8), dtype=torch.float32, device="cuda"))


# ---- 2. the score matrix -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrix16(gpu):
    """65 probes x 65 gallery faces at 16 x 16 / 64: features, and score_pairs on all 4225 materialised pairs — ONE reference for
    every sub-block (score_pairs gives a pair the same bits in every batch: tests/test_gpu_smallres_attack.py)"""
    import torch
    net = _net(16, 64)
    rng = np.random.RandomState(2)
    n = max(SIZES)
    Pr = torch.from_numpy(rng.randint(0, 256, (n, 16, 16, 3)).astype(np.float32)).cuda()
    Ga = torch.from_numpy(rng.randint(0, 256, (n, 16, 16, 3)).astype(np.float32)).cuda()
    ref = net.score_pairs(Pr.repeat_interleave(n, dim=0), Ga.repeat(n, 1, 1, 1), prescale=True).reshape(n, n, 2)
    assert float((ref[..., 1].max() - ref[..., 1].min())) > 1e-3                           # not a constant
    return net, net.features(Pr, prescale=True), net.features(Ga, prescale=True), ref


@pytest.mark.parametrize("G", SIZES)
@pytest.mark.parametrize("P", SIZES)
def test_score_matrix_equals_score_pairs(gpu, matrix16, P, G):
    import torch
    net, FP, FG, ref = matrix16
    both = net.score_matrix(FP[:P], FG[:G])
    assert tuple(both.shape) == (P, G, 2) and torch.equal(both, ref[:P, :G])
    for col in (0, 1):
        one = net.score_matrix(FP[:P], FG[:G], col=col)
        assert tuple(one.shape) == (P, G) and torch.equal(one, ref[:P, :G, col]), (P, G, col)


def test_score_matrix_at_32x32_2048_and_its_refusals(gpu):
    import torch
    net = _net(32, 2048)
    rng = np.random.RandomState(4)
    P, G = 33, 65
    Pr = torch.from_numpy(rng.randint(0, 256, (P, 32, 32, 3)).astype(np.float32)).cuda()
    Ga = torch.from_numpy(rng.randint(0, 256, (G, 32, 32, 3)).astype(np.float32)).cuda()
    ref = net.score_pairs(Pr.repeat_interleave(G, dim=0), Ga.repeat(P, 1, 1, 1), prescale=True).reshape(P, G, 2)
    FP, FG = net.features(Pr, prescale=True), net.features(Ga, prescale=True)
    out = torch.empty((P, G, 2), dtype=torch.float32, device="cuda")
    assert net.score_matrix(FP, FG, out=out) is out and torch.equal(out, ref)
    assert torch.equal(net.score_matrix(FP, FG, col=1), ref[..., 1]) and torch.equal(net.score_matrix(FP, FG, col=0), ref[..., 0])
    assert tuple(net.score_matrix(FP[:0], FG).shape) == (0, G, 2) and tuple(net.score_matrix(FP, FG[:0], col=1).shape) == (P, 0)
    with pytest.raises(ValueError):
        net.score_matrix(FP[:, :2040], FG)
    with pytest.raises(ValueError):
        net.score_matrix(FP, FG, col=2)
    # the size limit of one call (include/alink_hip.h: nL * nR * od <= 2^28) is refused before anything is launched or read
    lib = gpu.load()
    st = gpu.current_stream(net.device)
    assert lib.alink_smallres_score_features(net.h, gpu.ptr(FP), 16384, gpu.ptr(FG), 8193, 1, gpu.ptr(out), st) != 0
    assert lib.alink_smallres_score_features(net.h, gpu.ptr(FP), P, gpu.ptr(FG), G, 2, gpu.ptr(out), st) != 0       # no such column
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


# ---- 3. the row reduction ------------------------------------------------------------------------------------------------------
def _rows(G, C, rng):
    """five rows of G x C scores: many exact ties (few levels); 0.5 / 0.5 everywhere; the maximum in the LAST element; duplicate
    gallery entries (a short pattern repeated); continuous values"""
    levels = rng.randint(0, 4, (G, C)).astype(np.float32) / 4.0
    half = np.full((G, C), 0.5, np.float32)
    last = rng.rand(G, C).astype(np.float32) * 0.5
    last[G - 1, C - 1] = 0.75
    dup = np.tile(rng.rand(3, C).astype(np.float32), ((G + 2) // 3, 1))[:G]
    cont = rng.rand(G, C).astype(np.float32)
    return np.stack([levels, half, last, dup, cont])


def _numpy_identify(scores, col, true):
    P, G = scores.shape[:2]
    flat = scores.reshape(P, -1).argmax(axis=1)
    best = scores[:, :, col].argmax(axis=1)
    rank = np.full(P, -1, np.int64)
    for p in range(P):
        if 0 <= true[p] < G:
            order = np.argsort(-scores[p, :, col], kind="stable")
            rank[p] = int(np.nonzero(order == true[p])[0][0])
    return flat, best, rank


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 257, 1025])
def test_identify_rows_against_numpy(gpu, G, P):
    import torch
    from a_link_amd.smallres import identify_rows
    rng = np.random.RandomState(100 * G + P)
    for C in (2, 1):
        rows = _rows(G, C, rng)
        valid = int(rng.randint(0, G))
        if P == 5:                                       # the five kinds of row in one call; true: valid, -1, G (out of range), last, first
            cases = [(rows, [valid, -1, G, G - 1, 0])]
        else:                                            # P = 1: every kind of row on its own, with a valid, a negative and an out-of-range id
            cases = [(rows[k:k + 1], [t]) for k in range(5) for t in (valid, -1, G)]
        for col in range(C):
            for sc, true in cases:
                true = np.asarray(true, np.int32)
                dev = torch.from_numpy(np.ascontiguousarray(sc if C == 2 else sc[:, :, 0])).cuda()       # C = 1 as a (P, G) array
                flat, best, rank = identify_rows(dev, col=col, true_ids=true)
                want = _numpy_identify(sc, col, true)
                for got, ref, name in zip((flat, best, rank), want, ("flat_argmax", "best", "rank")):
                    assert got.dtype is torch.int32
                    assert np.array_equal(got.cpu().numpy().astype(np.int64), ref), (name, G, P, C, col, true.tolist())
    # outputs are optional one by one (NULL), and rank is not produced without true_ids
    sc = torch.from_numpy(_rows(G, 2, rng)[:P]).cuda().contiguous()
    flat, best, rank = identify_rows(sc, col=1)
    assert rank is None and np.array_equal(flat.cpu().numpy(), sc.cpu().numpy().reshape(P, -1).argmax(axis=1))
    lib = gpu.load()
    only = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    gpu.check(lib.alink_identify_rows(gpu.ptr(sc), P, G, 2, 1, None, None, gpu.ptr(only), None, gpu.current_stream(0)))
    assert torch.equal(only, best)
    assert lib.alink_identify_rows(gpu.ptr(sc), P, G, 2, 2, None, gpu.ptr(only), None, None, gpu.current_stream(0)) != 0      # col outside C
    assert lib.alink_identify_rows(gpu.ptr(sc), P, G, 2, 1, None, None, None, gpu.ptr(only), gpu.current_stream(0)) != 0      # rank without true


# ---- 4 / 5. end to end, and isolation ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def split16(gpu):
    """6 people x 3 images at 16 x 16 / 64; person 4's gallery image is a copy of person 1's (exact ties across the gallery)"""
    from a_link_amd import siamese
    student = siamese.SmallRes((16, 16, 3), (64,), "identify16", 0.1, seed=4)
    ws = student.siamese_net.get_weights()
    ws[14] = ws[14] * np.float32(8.0)
    student.siamese_net.set_weights(ws)
    rng = np.random.RandomState(5)
    people = [rng.randint(0, 256, (3, 16, 16, 3)).astype(np.float32) for _ in range(6)]
    people[4][0] = people[1][0]
    # the literal loop of code/ALINK_MTP.py:279-288, one probe per call, on score_pairs
    gal = np.stack([x[0] for x in people])
    rows, ids = [], []
    for i, person in enumerate(people):
        for x in person:
            rows.append(student.siamese_net.score_pairs(np.repeat(x[None], len(gal), axis=0), gal, prescale=True).cpu().numpy())
            ids.append(i)
    return student, people, np.stack(rows), np.asarray(ids)


def test_identify_equals_the_one_probe_per_call_loop(gpu, split16):
    from a_link_amd import alink_loop as AL
    student, people, scores, ids = split16
    want_flat = np.array([int(np.argmax(np.squeeze(s))) for s in scores])                  # predicted_id of the reference
    want_acc = sum(int(p == i) for p, i in zip(want_flat, ids)) / float(len(ids))
    _, want_best, want_rank = _numpy_identify(scores, 1, ids)
    assert scores[4 * 3, 1, 1] == scores[4 * 3, 4, 1]                                      # the duplicate gallery entry ties exactly
    probes = np.concatenate(people)
    gal = np.stack([x[0] for x in people])
    for cap in (64 << 20, 6 * 2 * 4 * 4, 1):             # one chunk; four probes per chunk (18 = 4 + 4 + 4 + 4 + 2); one probe per chunk
        got = student.identify(probes, gal, true_ids=ids, col=1, max_scores_bytes=cap)
        assert sorted(got) == ["best", "flat_argmax", "rank"] and all(v.dtype == np.int32 and v.shape == (18,) for v in got.values())
        assert np.array_equal(got["flat_argmax"], want_flat), cap
        assert np.array_equal(got["best"], want_best) and np.array_equal(got["rank"], want_rank), cap
        det = {}
        assert AL.top1_identification_gallery(student, people, max_scores_bytes=cap, details=det) == want_acc
        assert np.array_equal(det["true_ids"], ids) and np.array_equal(det["flat_argmax"], want_flat)
    assert sorted(student.identify(probes, gal)) == ["best", "flat_argmax"]               # no rank without true_ids
    st = AL.identification_stats(got["best"], got["rank"], ids, ks=(1, 6))
    assert st["rank1"] == float(np.mean(want_best == ids)) and st["cmc"][1] == st["rank1"] and st["cmc"][6] == 1.0


def test_features_and_identify_leave_the_model_alone(gpu, split16):
    student, people, _, ids = split16
    net = student.siamese_net
    rng = np.random.RandomState(9)
    X = [rng.randint(0, 256, (7, 16, 16, 3)).astype(np.float32) for _ in range(2)]
    w0, p0 = net.get_weights(), np.asarray(student.predict(X))
    net.features(np.concatenate(people), prescale=True)
    student.identify(np.concatenate(people), np.stack([x[0] for x in people]), true_ids=ids)
    assert all(np.array_equal(a, b) for a, b in zip(w0, net.get_weights()))
    assert np.array_equal(np.asarray(student.predict(X)), p0)


# ---- 6. the driver -------------------------------------------------------------------------------------------------------------
def _make_mtp(root, n_persons=5, seed=0):
    from PIL import Image
    rng = np.random.RandomState(seed)
    os.makedirs(root)
    for p in range(1, n_persons + 1):
        for suf in ("01_01_051_06.png", "02_01_051_06.png", "01_01_051_08.png", "02_01_051_08.png", "01_01_130_06.png"):
            Image.fromarray(rng.randint(0, 256, (64, 64, 3)).astype(np.uint8)).save(os.path.join(root, "%03d_%s" % (p, suf)))
    return root


def test_mtp_driver_with_gallery_eval(gpu, tmp_path, capsys):
    """ALINK_MTP.main --gallery_eval on the synthetic Multi-PIE tree of tests/test_gpu_driver.py: the run finishes, prints the
    reference's line and the extension's, and its top-1 is top1_identification_gallery's on the saved student"""
    from a_link_amd import ALINK_MTP, alink_loop, readMTP, siamese
    train, test = _make_mtp(str(tmp_path / "train")), _make_mtp(str(tmp_path / "test"), seed=1)
    models = str(tmp_path / "models")
    os.makedirs(models)
    common = ["--dataDirPrefix", train, "--testDir", test, "--quiet", "--lowRes", "32", "--noise", "gaussian,plain",
              "--out_model", os.path.join(models, "postALINK"), "--ensemble_basepath", os.path.join(models, "ensemble"),
              "--lowres_basemodel", os.path.join(models, "lowresModel"), "--pretrain_steps", "32", "--lowres_epochs", "1"]
    np.random.seed(0)
    assert ALINK_MTP.main(common) is None                                   # first run trains the low-res model and quits
    st = ALINK_MTP.main(common + ["--alink_bs", "2", "--batch_send", "4", "--disparity_ratio", "1.0", "--eps", "0.0",
                                  "--ft_epochs", "1", "--active_ratio", "4.0", "--gallery_eval"])
    out = capsys.readouterr().out
    assert "Top-1 accuracy : " in out and "Rank-1 on P(same) (extension) : " in out
    assert st.iterations >= 1 and 0.0 <= st.top1 <= 1.0 and 0.0 <= st.identification["rank1"] <= 1.0
    student = siamese.SmallRes((32, 32, 3), (2048,), os.path.join(models, "postALINK"), 1e-1)
    assert student.maybeLoadFromMemory()
    X_test = readMTP.readAllImages(test, (32, 32))
    assert len(X_test) == 5
    assert st.top1 == alink_loop.top1_identification_gallery(student, X_test)
