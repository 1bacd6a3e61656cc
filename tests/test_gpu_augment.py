"""GPU: --augment (reference code/helpers.py:114-141 behind code/ALINK_arc.py:233-238) through every layer.

  * alink_affine_warp (csrc/augment.hip) equals scipy.ndimage.affine_transform(mode='nearest') bit for bit, order 0 and 1;
  * helpers.augment_data equals a scipy-based restatement of the reference function (tests/test_augment_host.py) under
    the same seed: pixels, labels and the random state afterwards;
  * the loop with Flags(augment=True) equals literal reference-shaped loops (DFW, and MTP with its branch repaired), on
    one process and on two ranks, and the driver runs end to end with --augment."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

from test_augment_host import reference_augment_data

pytestmark = pytest.mark.gpu
SIZE = (32, 32)


def _scipy_warp(img, m, order):
    return np.stack([ndimage.affine_transform(img[..., ch], m[:, :2], m[:, 2], order=order, mode="nearest")
                     for ch in range(img.shape[-1])], axis=-1)


def _maps(rng, H, W, k):
    from a_link_amd import augment
    out = []
    for j in range(k):
        kind = j % 3
        if kind == 0:
            out.append(augment.affine_map(H, W, theta=rng.uniform(-20, 20)))
        elif kind == 1:
            out.append(augment.affine_map(H, W, shear=rng.uniform(-0.2, 0.2) if j % 2 else np.rad2deg(rng.uniform(-0.2, 0.2))))
        else:
            out.append(augment.affine_map(H, W, tx=rng.uniform(-0.2, 0.2) * H, ty=rng.uniform(-0.2, 0.2) * W))
    # extremes: half turns both ways, and shifts beyond the image that clamp every pixel to an edge
    out += [augment.affine_map(H, W, theta=180.0), augment.affine_map(H, W, theta=-180.0),
            augment.affine_map(H, W, tx=1.5 * H, ty=-2.5 * W), augment.affine_map(H, W, tx=-3.0 * H, ty=0.7 * W)]
    return np.stack(out)


@pytest.mark.parametrize("shape", [(112, 112, 3), (32, 32, 3), (112, 96, 3)])
@pytest.mark.parametrize("order", [0, 1])
def test_warp_equals_scipy(gpu, shape, order):
    """one gather launch: repeated sources, copy rows, NumPy and CUDA-tensor tables; every output row against scipy"""
    from a_link_amd import augment
    H, W, Cc = shape
    rng = np.random.RandomState(H + W + order)
    table = rng.randint(0, 256, (3,) + shape).astype(np.float32)
    table[0, :4] = rng.uniform(0, 255, (4, W, Cc))                  # non-integer pixels too
    maps = _maps(rng, H, W, 9)
    R = len(maps)
    src = rng.randint(0, 3, R)
    src[:3] = [2, 2, 0]
    copy = np.zeros(R, bool)
    copy[[1, 5]] = True
    got = augment.warp(table, src, maps, order, copy)
    assert isinstance(got, np.ndarray) and got.shape == (R,) + shape and got.dtype == np.float32
    for i in range(R):
        want = table[src[i]] if copy[i] else _scipy_warp(table[src[i]], maps[i], order)
        assert got[i].tobytes() == want.tobytes(), (i, np.abs(got[i] - want).max())
    dev = augment.warp(torch.from_numpy(table).cuda(), src, maps, order, copy)
    assert dev.is_cuda and torch.equal(dev.cpu(), torch.from_numpy(got))
    tiled = np.concatenate([table] * 5)[:R]
    same = augment.warp(tiled, None, maps, order)                    # no source rows: output i reads image i
    for i in (0, R - 1):
        assert same[i].tobytes() == _scipy_warp(tiled[i], maps[i], order).tobytes()
    empty = augment.warp(torch.from_numpy(table).cuda(), [], np.zeros((0, 2, 3)), order)
    assert tuple(empty.shape) == (0,) + shape and empty.is_cuda
    assert augment.warp(table, None, np.zeros((0, 2, 3)), order).shape == (0,) + shape


@pytest.mark.parametrize("factor,flags", [(1, (True, True, True)), (2, (True, False, True)), (1, (False, True, False))])
def test_augment_data_equals_reference(gpu, factor, flags):
    from a_link_amd import helpers
    rng = np.random.RandomState(factor)
    L = rng.randint(0, 256, (3, 64, 56, 3)).astype(np.float32)
    Rr = rng.randint(0, 256, (3, 64, 56, 3)).astype(np.float32)
    y = np.array([[1], [0], [1]])
    np.random.seed(21)
    (wl, wr), wy = reference_augment_data([L, Rr], y, factor, *flags)
    want_state = np.random.get_state()
    np.random.seed(21)
    (gl, gr), gy = helpers.augment_data([L, Rr], y, factor, *flags)
    got_state = np.random.get_state()
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1], want_state[1]) and got_state[2:] == want_state[2:]
    assert np.array_equal(gy, wy) and gy.shape == wy.shape
    assert gl.dtype == np.float32 and gl.tobytes() == wl.astype(np.float32).tobytes()
    assert gr.tobytes() == wr.astype(np.float32).tobytes()
    # CUDA tensors in -> CUDA tensors out, the same pixels
    np.random.seed(21)
    (tl, tr), ty = helpers.augment_data([torch.from_numpy(L).cuda(), torch.from_numpy(Rr).cuda()], y, factor, *flags)
    assert tl.is_cuda and torch.equal(tl.cpu(), torch.from_numpy(gl)) and torch.equal(tr.cpu(), torch.from_numpy(gr))


# ---- the loop: code/ALINK_arc.py:142-254 with the --augment branch, line for line -------------------------------------
def _people(n, seed, lo=2, hi=3):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (rng.randint(lo, hi + 1),) + SIZE + (3,)).astype(np.float32) for _ in range(n)]


def _build(seed, noises=("gaussian", "speckle")):
    from a_link_amd import committee, noise, siamese
    conv = siamese.ArcFace(SIZE, "synthetic:r18:3")
    student = siamese.SiameseNetwork((512,), "student", 0.1, seed=seed)
    ens = [siamese.SiameseNetwork((512,), "ens%d" % i, 0.1, seed=100 + i) for i in range(2)]
    nz = [noise.get_relevant_noise(n)(model=student, sess=None, feature_model=conv) for n in noises]
    for i, z in enumerate(nz):
        z._seed, z._calls = 1000 + i, 0
    return conv, student, ens, committee.Bagging(ens, nz), nz


def _select(ens, dps, batch_y, flags, col):
    """code/ALINK_arc.py:167-198 (np.argsort made stable; Set -> sorted set)"""
    mis = []
    for dp in dps:
        d = [-np.absolute(dp[j][col] - ens[j][col]) for j in range(len(dp))]
        mis.append(np.argsort(d, kind="stable")[:int(len(d) * flags.disparity_ratio)])
    works = set(mis[0].tolist())
    for m in mis[1:]:
        works &= set(m.tolist())
    q, active = [], 0
    for j in sorted(works):
        e = ens[j][col]
        if e <= 0.5 - flags.eps or e >= 0.5 + flags.eps:
            active += 1
            if (e >= 0.5) == (batch_y[j][0] >= 0.5):
                q.append(j)
    return q, active


def _literal_loop(flags, conv, bag, nz, student, X_plain_raw, X_dig_post, dataGen, col, mtp_low=None):
    """code/ALINK_arc.py:142-254 with FLAGS.augment (:233-238); mtp_low = (image_res, low_res): the shape of
    code/ALINK_MTP.py:150-266 instead — features of the high-res pairs for the committee, the student on low-res pixels,
    and the augment branch of :244-248 as it evidently meant (both sides' low-res rows; the reference names an undefined
    batch_x_left twice)"""
    from a_link_amd import alink_loop as AL, helpers, noise, pairs
    tl, tr, ty = np.array([]), np.array([]), np.array([])
    ACTIVE, UN, sets, fts = 0, 0, [], 0
    for ii in range(0, len(X_dig_post), flags.alink_bs):
        if mtp_low is None:
            batch_x, batch_y = pairs.createMiniBatch(X_plain_raw[ii:ii + flags.alink_bs], X_dig_post[ii:ii + flags.alink_bs])
            feats = [conv.process(p) for p in batch_x]
            student_x = feats
            attack_res, attack_labels = SIZE, None
        else:
            batch_x, batch_y = AL.createMiniBatchMTP(X_dig_post[ii:ii + flags.alink_bs])
            feats = [conv.process(np.asarray(noise.resize_images(p, mtp_low[0]))) for p in batch_x]
            student_x = [np.asarray(noise.resize_images(p, mtp_low[1])) for p in batch_x]      # batch_x_lowres
            attack_res, attack_labels = mtp_low[1], True
        UN += len(batch_x[0])
        ens = bag.predict(feats)
        m1 = np.argmax(ens, axis=1)
        noisy = bag.attackModel(batch_x, attack_res, helpers.one_hot(m1, 2) if attack_labels else m1)
        if mtp_low is None:
            noisy = [[conv.process(p) for p in part] for part in noisy]
        else:
            noisy = [[np.asarray(p) for p in part] for part in noisy]
        dps = [student.predict([noisy[0][j], noisy[1][j]]) for j in range(len(nz))]
        q, active = _select(ens, dps, batch_y, flags, col)
        ACTIVE += active
        sets.append(list(q))
        if not q:
            continue
        inter = np.array([ens[i][col] for i in q])
        mp = int(len(inter) / float(len(nz)))
        parts_l = [noisy[0][i][q[i * mp:(i + 1) * mp]] for i in range(len(nz))]
        parts_r = [noisy[1][i][q[i * mp:(i + 1) * mp]] for i in range(len(nz))]
        parts_y = [helpers.roundoff(inter)[i * mp:(i + 1) * mp] for i in range(len(nz))]
        tl = np.concatenate(([tl] if ty.shape[0] > 0 else []) + parts_l)
        tr = np.concatenate(([tr] if ty.shape[0] > 0 else []) + parts_r)
        ty = np.concatenate(([ty] if ty.shape[0] > 0 else []) + parts_y)
        if ty.shape[0] >= flags.batch_send:
            (ol, orr), oy = next(dataGen)
            for _ in range(flags.mixture_ratio - 1):
                t, yy = next(dataGen)
                ol, orr, oy = np.concatenate((ol, t[0])), np.concatenate((orr, t[1])), np.concatenate((oy, yy))
            assert flags.augment
            if mtp_low is None:
                batch_x_aug, batch_y_aug = reference_augment_data([batch_x[0][q], batch_x[1][q]], helpers.roundoff(inter), 1)
                batch_x_aug = [conv.process(p.astype(np.float32)) for p in batch_x_aug]
            else:
                batch_x_aug, batch_y_aug = reference_augment_data([student_x[0][q], student_x[1][q]], helpers.roundoff(inter), 1)
            tl = np.concatenate((tl, batch_x_aug[0], ol))
            tr = np.concatenate((tr, batch_x_aug[1], orr))
            ty = np.concatenate((ty, batch_y_aug, oy))
            student.finetune([tl, tr], ty, flags.ft_epochs, 16, 0)
            fts += 1
            tl, tr, ty = np.array([]), np.array([]), np.array([])
        if int(flags.active_ratio * UN) <= ACTIVE:
            break
    return ACTIVE, UN, sets, fts


def _spy_sets(AL):
    sets = []
    orig = AL.selection.select_queries

    def spy(*a, **k):
        r = orig(*a, **k)
        sets.append(list(r[0]))
        return r
    AL.selection.select_queries = spy
    return sets, lambda: setattr(AL.selection, "select_queries", orig)


@pytest.mark.parametrize("col", [0, 1])
def test_augment_loop_equals_reference_shaped_loop(gpu, col, tmp_path):
    """run_alink_dfw with Flags(augment=True) against code/ALINK_arc.py:142-254 restated with its augment branch (scipy
    resampling, every augmented image embedded): query sets, counts and the student's weights bit for bit"""
    from a_link_amd import alink_loop as AL, pairs
    flags = AL.Flags(alink_bs=3, batch_send=6, disparity_ratio=0.6, eps=0.0005, ft_epochs=2, mixture_ratio=2,
                     out_model=str(tmp_path / "post"), augment=True)
    X_plain, X_dig = _people(6, 1), _people(6, 2)
    results = []
    for which in ("library", "literal"):
        conv, student, ens, bag, nz = _build(7)
        feats_plain = [conv.process(p) for p in X_plain]
        gen = pairs.getGenerator(pairs.getNormalGenerator(feats_plain, 8), pairs.getNormalGenerator(feats_plain, 8),
                                 pairs.getImposterGenerator(feats_plain, feats_plain, 8), 8)
        np.random.seed(5)
        if which == "library":
            sets, undo = _spy_sets(AL)
            try:
                st = AL.run_alink_dfw(flags, conv, bag, nz, student, X_plain, X_dig, gen, SIZE, col=col, verbose=0)
            finally:
                undo()
            assert st.recalibrations == 0
            results.append((st.active_count, st.un_size, sets, st.finetunes, student.siamese_net.get_weights()))
        else:
            a, u, sets, fts = _literal_loop(flags, conv, bag, nz, student, X_plain, X_dig, gen, col)
            results.append((a, u, sets, fts, student.siamese_net.get_weights()))
    lib, lit = results
    assert lib[:4] == lit[:4]
    assert lib[3] >= 1, "test data must trigger at least one fine-tune"
    for a, b in zip(lib[4], lit[4]):
        assert np.array_equal(a, b)


def test_augment_mtp_loop_equals_repaired_reference_branch(gpu, tmp_path):
    """run_alink_mtp with Flags(augment=True): every fine-tune set holds 4 |q| augmented low-res rows where the clean
    |q| rows would be, and the student's weights equal those of ALINK_MTP.py's loop restated with the repaired branch"""
    from a_link_amd import alink_loop as AL, committee, noise, pairs, siamese
    low = (16, 16)
    rng = np.random.RandomState(3)
    people = [rng.randint(0, 256, (2, 40, 40, 3)).astype(np.float32) for _ in range(6)]
    flags = AL.Flags(alink_bs=3, batch_send=4, disparity_ratio=1.0, eps=0.0, ft_epochs=1, active_ratio=2.0,
                     out_model=str(tmp_path / "post"), augment=True)
    results = []
    for which in ("library", "literal"):
        conv = siamese.ArcFace(SIZE, "synthetic:r18:3")
        student = siamese.SmallRes(low + (3,), (64,), str(tmp_path / ("lowres_" + which)), 0.1, seed=2)
        ens = [siamese.SiameseNetwork((512,), "e%d" % i, 0.1, seed=50 + i) for i in range(2)]
        nz = [noise.Gaussian(seed=1), noise.Noise()]
        bag = committee.Bagging(ens, nz)
        gen = pairs.getGeneratorMTP(pairs.getNormalGenerator(people, 16), 8, resize_res=low)
        np.random.seed(0)
        if which == "library":
            sets, undo = _spy_sets(AL)
            seen = []
            orig_ft = student.finetune

            def ft(X, y, *a, **k):
                seen.append((len(sets), np.asarray(X[0]).copy(), np.asarray(X[1]).copy(), np.asarray(y).copy()))
                return orig_ft(X, y, *a, **k)
            student.finetune = ft
            try:
                st = AL.run_alink_mtp(flags, conv, bag, nz, student, people, gen, SIZE, low, verbose=0)
            finally:
                undo()
            assert st.finetunes >= 1 and seen[0][0] == 1, "test data must fine-tune in the first iteration"
            # the first set: the pending noisy rows (n_noise * mp), then 4 |q| augmented rows — original, rotation, shear,
            # shift per queried pair, the originals being the clean low-res rows — then the generator's rows
            q = sets[0]
            pend = len(nz) * (len(q) // len(nz))
            bx, by = AL.createMiniBatchMTP(people[:flags.alink_bs])
            for s in (0, 1):
                clean = np.asarray(noise.resize_images(bx[s], low))[q]
                aug = seen[0][1 + s][pend:pend + 4 * len(q)]
                assert np.array_equal(aug[0::4], clean)
                assert all(not np.array_equal(aug[k::4], clean) for k in (1, 2, 3))
            assert np.array_equal(seen[0][3][pend:pend + 4 * len(q)].ravel(), np.repeat(by[q].ravel(), 4))
            results.append((st.active_count, st.un_size, sets, st.finetunes, student.siamese_net.get_weights()))
        else:
            a, u, sets, fts = _literal_loop(flags, conv, bag, nz, student, None, people, gen, 0, mtp_low=(SIZE, low))
            results.append((a, u, sets, fts, student.siamese_net.get_weights()))
    lib, lit = results
    assert lib[:4] == lit[:4]
    for a, b in zip(lib[4], lit[4]):
        assert np.array_equal(a, b)


# ---- two ranks on one card (the pattern of test_gpu_distributed.test_multirank_alink_loop_equals_single_process_loop) ----
def _rank_run(group, rank, tmp):
    from a_link_amd import alink_loop as AL, committee, noise, pairs, siamese
    flags = AL.Flags(alink_bs=3, batch_send=6, disparity_ratio=0.6, eps=0.0005, ft_epochs=2, mixture_ratio=2,
                     out_model=os.path.join(tmp, "aug%d" % rank), augment=True)
    X_plain, X_dig = _people(6, 1), _people(6, 2)
    conv = siamese.ArcFace(SIZE, "synthetic:r18:3")
    conv.calibrate(np.concatenate(X_plain + X_dig))
    student = siamese.SiameseNetwork((512,), "student", 0.1, seed=7)
    ens = [siamese.SiameseNetwork((512,), "ens%d" % i, 0.1, seed=100 + i) for i in range(2)]
    # rank 0 carries the single-process run's seeds; the other rank starts from different noise streams and host randomness
    nz = [noise.get_relevant_noise(n)(model=student, sess=None, feature_model=conv, seed=1000 + i + 50 * rank)
          for i, n in enumerate(("gaussian", "speckle"))]
    bag = committee.Bagging(ens, nz)
    feats_plain = [conv.process(p) for p in X_plain]
    gen = pairs.getGenerator(pairs.getNormalGenerator(feats_plain, 8), pairs.getNormalGenerator(feats_plain, 8),
                             pairs.getImposterGenerator(feats_plain, feats_plain, 8), 8)
    np.random.seed(5 + 31 * rank)
    sets, undo = _spy_sets(AL)
    try:
        st = AL.run_alink_dfw(flags, conv, bag, nz, student, X_plain, X_dig, gen, SIZE, col=0, verbose=0, group=group)
    finally:
        undo()
    return {"counts": np.array([st.active_count, st.un_size, st.finetunes, st.recalibrations]),
            "sets": np.array([len(s) for s in sets] + sum(sets, [])),
            "w": np.concatenate([w.ravel() for w in student.siamese_net.get_weights()])}


def _rank_worker(rank, world, port, path, tmp):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        import a_link_amd  # noqa: F401
        np.savez(path % rank, **_rank_run(dist.group.WORLD, rank, tmp))
    finally:
        dist.destroy_process_group()


def test_augment_loop_on_two_ranks_equals_single_process(gpu, tmp_path):
    import socket
    import torch.multiprocessing as mp
    want = _rank_run(None, 0, str(tmp_path))
    assert want["counts"][2] >= 1, "test data must fine-tune"
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    path = str(tmp_path / "aug_rank%d.npz")
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, path, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0
    for r in range(2):
        z = np.load(path % r)
        assert np.array_equal(z["counts"], want["counts"]), (r, z["counts"], want["counts"])
        assert np.array_equal(z["sets"], want["sets"]), r
        assert np.array_equal(z["w"], want["w"]), (r, np.abs(z["w"] - want["w"]).max())


def test_driver_runs_with_augment(gpu, tmp_path):
    """ALINK_arc.main(... --augment) end to end on the synthetic DFW tree of tests/test_gpu_driver.py"""
    from a_link_amd import ALINK_arc
    from test_gpu_driver import _make_dfw
    root = _make_dfw(str(tmp_path))
    models = str(tmp_path / "models")
    os.makedirs(models)
    common = ["--dataDirPrefix", root, "--arcface_model", "synthetic:r18:2", "--quiet",
              "--out_model", os.path.join(models, "postALINK"), "--ensemble_basepath", os.path.join(models, "ensemble"),
              "--disguised_basemodel", os.path.join(models, "disguisedModel"), "--pretrain_steps", "64",
              "--dig_epochs", "1", "--undig_epochs", "1", "--noise", "gaussian,speckle"]
    np.random.seed(0)
    assert ALINK_arc.main(common + ["--train_disguised_model"]) is None
    st = ALINK_arc.main(common + ["--alink_bs", "3", "--batch_send", "2", "--disparity_ratio", "1.0", "--eps", "0.0",
                                  "--ft_epochs", "1", "--active_ratio", "4.0", "--augment"])
    assert os.path.exists(os.path.join(models, "postALINK.h5"))
    assert st.iterations >= 1 and st.finetunes >= 1
