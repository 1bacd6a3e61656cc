"""GPU: the rectangular k-nearest-neighbour search and the CAL score on device (alink_knn_rect, alink_cal_score, knn_rect.hip;
a-link_amd/cal.py) — bit equality with the host rule (cal.knn_rect) on small-integer rows around every size the kernel has, a
reference set where everything ties, the tie to alink_knn, the pair form against the row form, real-valued rows within the
float32 bound of a D-term chain, non-finite rows on either side, the score against the host's float64 under a derived tolerance,
the selection against the host, its Bagging form, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_typiclust_host import int_rows, same_lists

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set_dev(rows):
    """a row set for the device forms: NumPy arrays are copied over, tensors are taken as they are"""
    if isinstance(rows, tuple):
        return tuple(_set_dev(a) for a in rows)
    return rows if isinstance(rows, torch.Tensor) else _dev(rows)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _run(queries, references, k):
    """alink_knn_rect with every output -> (idx, d2, found) as NumPy arrays"""
    from a_link_amd import cal
    idx, d2, found = cal.knn_rect_device(_set_dev(queries), _set_dev(references), k)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and found.dtype == torch.int32
    assert idx.shape == d2.shape and idx.shape[1] == k and found.shape == (idx.shape[0],)
    return idx.cpu().numpy(), d2.cpu().numpy(), found.cpu().numpy()


def _check_against_host(Q, Cm, k, got):
    from a_link_amd import cal
    want = cal.knn_rect(Q, Cm, k)
    assert same_lists(got, want) is None, same_lists(got, want)
    assert np.array_equal(np.isnan(got[1]), got[0] < 0)                    # unfilled slots: -1 and NaN
    assert (got[2] <= min(k, len(Cm))).all()


# (N, M, D, K).  The kernel's sizes: 128 queries a workgroup (32 a wave), 128 references a tile in blocks of 32, 32 columns a chunk;
# lists of 8, 16 and 32; 16-byte loads where D is a multiple of 4.
INT_SHAPES = [(1, 1, 1, 1), (1, 33, 33, 20), (2, 2, 3, 5), (33, 1, 130, 1), (33, 31, 32, 32), (33, 32, 33, 5), (127, 33, 3, 20),
              (128, 127, 32, 8), (128, 128, 1, 32), (129, 129, 33, 16), (129, 257, 130, 1), (257, 300, 130, 20), (257, 5, 1, 32),
              (300, 128, 3, 32), (300, 129, 32, 5), (300, 300, 33, 20), (5, 300, 7, 17), (130, 40, 40, 9)]


@pytest.mark.parametrize("N,M,D,K", INT_SHAPES)
def test_integer_rows_bit_equal_to_the_host_rule(gpu, N, M, D, K):
    """rows in -4 .. 4: every product, score and d2 is an integer far below 2^24 — exact in any order, so idx, d2 and found must
    equal the host's bit for bit, ties (there are many) included"""
    Q, Cm = int_rows(N, D), int_rows(M, D, seed=3)
    got = _run(Q, Cm, K)
    _check_against_host(Q, Cm, K, got)
    assert (got[2] == min(K, M)).all()
    assert _same_bits(_run(Q, Cm, K), got)                                 # two runs of a call


def test_a_reference_set_of_identical_rows(gpu):
    """everything ties: the lists are the lowest indices 0 .. K - 1 for every query"""
    for N, M, D, K in ((300, 200, 7, 20), (129, 130, 32, 32), (20, 5, 3, 8)):
        Q, Cm = int_rows(N, D), np.tile(int_rows(1, D, seed=9), (M, 1))
        idx, d2, found = _run(Q, Cm, K)
        w = min(K, M)
        assert (idx[:, :w] == np.arange(w)[None, :]).all() and (idx[:, w:] == -1).all() and (found == w).all()
        assert np.array_equal(d2[:, :w], np.repeat(((Q - Cm[0]) ** 2).sum(axis=1, dtype=np.float32)[:, None], w, axis=1))


@pytest.mark.parametrize("N,D,K", [(300, 33, 20), (257, 130, 31), (129, 32, 7), (33, 3, 15)])
def test_a_set_against_itself_gives_alink_knns_lists(gpu, N, D, K):
    """references = queries on integer rows: a row's rectangular list of K + 1 without itself (or, where it is absent, without
    its last entry) is alink_knn's list of K, bit for bit in idx and d2"""
    from a_link_amd import typiclust
    X = int_rows(N, D)
    ridx, rd2, rfound = _run(X, X, K + 1)
    sq = typiclust.knn_device(_dev(X), K)
    sidx, sd2 = sq[0].cpu().numpy(), sq[1].cpu().numpy()
    assert (rfound == min(K + 1, N)).all()
    kept_idx, kept_d2 = np.empty_like(sidx), np.empty_like(sd2)
    for n in range(N):
        keep = [p for p in range(K + 1) if ridx[n, p] != n]
        keep = keep[:K]
        kept_idx[n], kept_d2[n] = ridx[n, keep], rd2[n, keep]
    assert np.array_equal(kept_idx, sidx) and np.array_equal(_bits(kept_d2), _bits(sd2))
    assert (ridx == np.arange(N)[:, None]).any(axis=1).mean() > 0.5        # most rows do find themselves


@pytest.mark.parametrize("D", [33, 64])
def test_the_first_neighbour_is_the_k_means_assignment(gpu, D):
    """real-valued rows: alink_kmeans with no update step assigns every row to argmin_j fma(-2, x . c_j, |c_j|^2), ties to the
    lower index, and so does the first column of alink_knn_rect at K = 1 against the centres as a row table — one fmaf chain
    behind both (pool_tile.h), so the two agree index for index, not within a band.  300 rows against 130 centres: two candidate
    tiles, the second with one partial MFMA block; D = 33 takes scalar loads and a partial chunk, D = 64 the 16-byte loads."""
    from a_link_amd import cluster
    rng = np.random.RandomState(1300 + D)
    X, Cm = rng.randn(300, D).astype(np.float32), rng.randn(130, D).astype(np.float32)
    X, Cm = X[np.isfinite(X).all(axis=1)], Cm[np.isfinite(Cm).all(axis=1)]
    assign = cluster.kmeans_device(_dev(X), len(Cm), iters=0, centres=_dev(Cm))["assign"].cpu().numpy()
    idx, _, found = _run(X, Cm, 1)
    assert (found == 1).all() and np.array_equal(assign, idx[:, 0])
    assert len(np.unique(assign)) > 32                                     # the assignment is spread over both tiles' blocks


@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D):
    rng = np.random.RandomState(D)
    P, G, N, M, K = 60, 9, 300, 140, 20
    li, ri = rng.randint(0, P, N).astype(np.int32), rng.randint(0, G, N).astype(np.int32)
    cli, cri = rng.randint(0, P, M).astype(np.int32), rng.randint(0, G, M).astype(np.int32)
    for integer in (True, False):
        def table(rows):
            return rng.randint(-2, 3, (rows, D)).astype(np.float32) if integer else rng.randn(rows, D).astype(np.float32)
        L, R, L2, R2 = table(P), table(G), table(P), table(G)
        for cl, cr in ((L, R), (L2, R2)):                                  # shared tables, tables of the references' own
            Q = np.abs(L[li] - R[ri])                                       # one rounded subtraction: the bits the on-the-fly row holds
            Cm = np.abs(cl[cli] - cr[cri])
            pair, row = _run((L, R, li, ri), (cl, cr, cli, cri), K), _run(Q, Cm, K)
            assert _same_bits(pair, row), (integer, cl is L)
            if integer:
                _check_against_host(Q, Cm, K, pair)
    # a table 4 bytes off the 16-byte alignment on either side (the scalar loads) against the aligned run
    Q, Cm = rng.randn(N, D).astype(np.float32), rng.randn(M, D).astype(np.float32)
    want = _run(Q, Cm, K)

    def off(a):
        buf = torch.empty(a.size + 1, device="cuda")
        buf[1:] = _dev(a).reshape(-1)
        t = buf[1:].view(a.shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    assert _same_bits(_run(off(Q), _dev(Cm), K), want)
    assert _same_bits(_run(_dev(Q), off(Cm), K), want)
    assert _same_bits(_run((off(Q), _dev(np.zeros_like(Q)), _dev(np.arange(N, dtype=np.int32)), _dev(np.arange(N, dtype=np.int32))),
                           (_dev(Cm), off(np.zeros_like(Cm)), _dev(np.arange(M, dtype=np.int32)), _dev(np.arange(M, dtype=np.int32))), K),
                      _run(np.abs(Q), np.abs(Cm), K))


def rect_within_float32_bound(Q, Cm, k, idx, found):
    """test_typiclust_host.within_float32_bound for two sets.  In float64: s(n, j) = |c_j|^2 - 2 q_n . c_j and
    E(n, j) = g (|c_j|^2 + 2 |q_n| |c_j|), g = (D + 8) 2^-24, the bound of a D-term float32 chain.  A result passes when, for every
    query, found = min(k, M), the reported references are distinct, unfilled slots are -1, every reported j and every unreported i
    satisfy s(n, j) <= s(n, i) + E(n, j) + E(n, i), and consecutive entries satisfy the same.  No row is exempt.
    -> (failures, queries whose set differs from the float64 set, largest excess as a fraction of its bound)"""
    Q, Cm = np.asarray(Q, np.float64), np.asarray(Cm, np.float64)
    N, D = Q.shape
    M = len(Cm)
    g = (D + 8) * 2.0 ** -24
    cn, qnorm = (Cm * Cm).sum(axis=1), np.sqrt((Q * Q).sum(axis=1))
    S = cn[None, :] - 2.0 * (Q @ Cm.T)
    E = g * (cn[None, :] + 2.0 * qnorm[:, None] * np.sqrt(cn)[None, :])
    fails, differ, worst = [], 0, -np.inf
    for n in range(N):
        f = int(found[n])
        rep = np.asarray(idx[n, :f], np.int64)
        if f != min(k, M):
            fails.append("query %d: found %d of min(%d, %d)" % (n, f, k, M))
            continue
        if (np.asarray(idx[n, f:]) != -1).any():
            fails.append("query %d: an unfilled slot is not -1" % n)
        if len(set(rep.tolist())) != f or rep.min() < 0 or rep.max() >= M:
            fails.append("query %d: reports a reference twice or one that does not exist" % n)
            continue
        true = np.argsort(S[n], kind="stable")[:f]
        differ += set(true.tolist()) != set(rep.tolist())
        rest = np.setdiff1d(np.arange(M), rep)
        if rest.size:
            room = E[n, rep][:, None] + E[n, rest][None, :]
            gap = S[n, rep][:, None] - S[n, rest][None, :]
            worst = max(worst, (gap / room).max())
            if (gap > room).any():
                fails.append("query %d: reports a reference %.3g bounds behind one it leaves out" % (n, (gap / room).max()))
        if f > 1:
            step = S[n, rep[:-1]] - S[n, rep[1:]]
            room = E[n, rep[:-1]] + E[n, rep[1:]]
            worst = max(worst, (step / room).max())
            if (step > room).any():
                fails.append("query %d: list out of order by %.3g bounds" % (n, (step / room).max()))
    return fails, differ, worst


def test_real_valued_rows_within_the_float32_bound(gpu):
    """300 x 128 against 200 x 128 and 260 x 512 against 140 x 512, K = 10, under rect_within_float32_bound; d2 within g of the
    float64 distance.  Measured on one MI355X: no query's set differs from the float64 set in either case; the largest excess
    is -0.144 / -0.0687 of its bound — negative: even the closest pair of scores stands in its float64 order."""
    rng = np.random.RandomState(14)
    cases = [("300 x 128 against 200 x 128", rng.randn(300, 128).astype(np.float32), rng.randn(200, 128).astype(np.float32)),
             ("260 x 512 against 140 x 512", (rng.randn(260, 512) * rng.uniform(0.5, 2.0, (260, 1))).astype(np.float32),
              (rng.randn(140, 512) * rng.uniform(0.5, 2.0, (140, 1))).astype(np.float32))]
    for name, Q, Cm in cases:
        idx, d2, found = _run(Q, Cm, 10)
        fails, differ, worst = rect_within_float32_bound(Q, Cm, 10, idx, found)
        print("%s: %d queries' sets differ from the float64 sets; largest excess %.3g of its bound" % (name, differ, worst))
        assert not fails, fails[:3]
        own = ((Q.astype(np.float64)[:, None, :] - Cm.astype(np.float64)[idx]) ** 2).sum(axis=2)
        assert (np.abs(d2 - own) <= (Q.shape[1] + 8) * 2.0 ** -24 * own).all()
    # the predicate is not vacuous: the k-th neighbour replaced by the one two ranks behind fails it
    want = np.argsort(((Cm ** 2).sum(axis=1)[None, :] - 2.0 * Q.astype(np.float64) @ Cm.astype(np.float64).T), axis=1, kind="stable")
    mutant = np.concatenate([want[:, :9], want[:, 11:12]], axis=1).astype(np.int32)
    assert rect_within_float32_bound(Q, Cm, 10, mutant, found)[0]


def test_non_finite_rows_on_either_side(gpu):
    """a NaN row and a +inf row among the queries: no neighbours; among the references: nobody's neighbour; every other row's list
    as if those rows were absent"""
    N, M, D, K = 200, 150, 33, 20
    Q, Cm = int_rows(N, D), int_rows(M, D, seed=2)
    qkeep, ckeep = np.ones(N, bool), np.ones(M, bool)
    qkeep[[5, 130]] = False
    ckeep[[0, 77, 149]] = False
    Q[5, 7], Q[130, 32] = np.nan, np.inf
    Cm[0, 0], Cm[77, 32], Cm[149, 5] = np.inf, np.nan, -np.inf
    idx, d2, found = _run(Q, Cm, K)
    _check_against_host(Q, Cm, K, (idx, d2, found))
    assert found[[5, 130]].tolist() == [0, 0] and (idx[[5, 130]] == -1).all() and np.isnan(d2[[5, 130]]).all()
    assert not np.isin(idx, [0, 77, 149]).any() and (found[qkeep] == K).all()
    sub = _run(Q[qkeep], Cm[ckeep], K)
    back = np.flatnonzero(ckeep)
    assert np.array_equal(back[sub[0]], idx[qkeep]) and np.array_equal(_bits(sub[1]), _bits(d2[qkeep]))
    # fewer live references than K: found < K, the tail -1 and NaN
    few = Cm[[0, 1, 77, 2, 149]]
    idx, d2, found = _run(Q, few, 8)
    _check_against_host(Q, few, 8, (idx, d2, found))
    assert (found[qkeep] == 2).all() and set(idx[qkeep][:, :2].ravel().tolist()) == {1, 3} and (idx[:, 2:] == -1).all()


# ---- the score -------------------------------------------------------------------------------------------------------------
def _softmax32(z):
    z = z.astype(np.float32)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def score_tolerance(p, q, idx, want):
    """|got - want| <= 2^-24 |want| + 16 2^-52 A, A = the mean over the found slots of sum_c q (|log q| + |log p'|): one float32
    rounding of the output, and a few units in the last place of float64 per logarithm and per sum, over the terms"""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    lp = np.abs(np.log(np.where(p > 2.0 ** -126, p, 2.0 ** -126)))
    with np.errstate(divide="ignore", invalid="ignore"):
        lq = np.where(q > 0, np.abs(np.log(q)), 0.0)
    A = np.zeros(len(p))
    for n in range(len(p)):
        js = idx[n][idx[n] >= 0]
        if len(js):
            A[n] = np.mean([(q[j] * (lq[j] + lp[n])).sum() for j in js])
    return 2.0 ** -24 * np.abs(want.astype(np.float64)) + 16 * 2.0 ** -52 * A


def _score_case(C, seed, N=500, M=90, K=10):
    rng = np.random.RandomState(seed)
    p, q = _softmax32(rng.randn(N, C) * 4), _softmax32(rng.randn(M, C) * 4)
    hot = np.zeros((1, C), np.float32)
    hot[0, 0] = 1
    p[::7], q[::5] = hot, np.roll(hot, C - 1, axis=1)                      # rows saturated to exact 0 and 1, on both sides
    p[3::7] = np.roll(hot, 1 % C, axis=1)
    idx = np.stack([rng.permutation(M)[:K] for _ in range(N)]).astype(np.int32)
    idx[1::4, rng.randint(1, K):] = -1                                     # found < K
    idx[2::9] = -1                                                         # found = 0
    return p, q, idx


@pytest.mark.parametrize("C", [2, 3, 7])
def test_cal_score_equals_the_host_float64_rule(gpu, C):
    """the tolerance is derived, not tuned (score_tolerance); a float32 evaluation of the rule fails it by orders of magnitude"""
    from a_link_amd import cal
    p, q, idx = _score_case(C, 40 + C)
    want = cal.cal_scores(p, q, idx)
    got = cal.cal_scores_device(_dev(p), _dev(q), _dev(idx)).cpu().numpy()
    tol = score_tolerance(p, q, idx, want)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("C = %d: largest |got - want| / tolerance = %.3g" % (C, (err / np.maximum(tol, 1e-300))[tol > 0].max()))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert (err <= tol).all(), (int((err > tol).sum()), float((err / np.maximum(tol, 1e-300)).max()))
    assert (got[2::9] == 0).all() and got.max() > 30                       # found = 0 scores 0; a floored zero of p stays finite, and large
    # a float32 evaluation of the same rule, for the size of the bound
    f32 = np.zeros(len(p), np.float32)
    lp32 = np.log(np.maximum(p, np.float32(2.0 ** -126)))
    with np.errstate(divide="ignore", invalid="ignore"):
        lq32 = np.log(q)
    for n in range(len(p)):
        js = idx[n][idx[n] >= 0]
        t = np.float32(0)
        for j in js:
            for c in range(C):
                if q[j, c] > 0:
                    t = np.float32(t + q[j, c] * np.float32(lq32[j, c] - lp32[n, c]))
        f32[n] = t / np.float32(len(js)) if len(js) else 0
    over = np.abs(f32.astype(np.float64) - want)[tol > 0] / tol[tol > 0]
    print("C = %d: a float32 evaluation misses the tolerance in %d of %d rows, by up to %.3g times" % (C, int((over > 1).sum()), len(over), over.max()))
    assert (over > 1).any()
    assert np.array_equal(cal.cal_scores_device(_dev(p), _dev(q), _dev(idx)).cpu().numpy(), got)


def test_cal_device_picks_equal_the_hosts_on_integer_rows(gpu):
    from a_link_amd import cal
    rng = np.random.RandomState(6)
    N, M, D, K = 400, 37, 12, 10
    rows, lab = int_rows(N, D), int_rows(M, D, seed=4)
    levels = np.array([[0.5, 0.5], [0.25, 0.75], [0.875, 0.125], [1.0, 0.0], [0.0, 1.0], [0.0625, 0.9375]], np.float32)
    p_pool, p_lab = levels[rng.randint(0, 6, N)], levels[rng.randint(0, 6, M)]
    want, wscores = cal.cal(rows, lab, p_pool, p_lab, 25, k_nn=K)
    picks, info = cal.cal_device(_dev(rows), _dev(lab), _dev(p_pool), _dev(p_lab), 25, k_nn=K)
    assert picks.dtype == torch.int32 and picks.is_cuda and np.array_equal(picks.cpu().numpy(), want)
    hidx = cal.knn_rect(rows, lab, K)
    assert same_lists((info["idx"].cpu().numpy(), info["d2"].cpu().numpy(), info["found"].cpu().numpy()), hidx) is None
    got = info["scores"].cpu().numpy()
    assert (np.abs(got.astype(np.float64) - wscores) <= score_tolerance(p_pool, p_lab, hidx[0], wscores)).all()
    # excluded rows are never picked; the batch is clipped to what is left
    ex = want[:5]
    picks2, _ = cal.cal_device(_dev(rows), _dev(lab), _dev(p_pool), _dev(p_lab), 25, k_nn=K, exclude=ex)
    assert np.array_equal(picks2.cpu().numpy(), cal.cal(rows, lab, p_pool, p_lab, 25, k_nn=K, exclude=ex)[0])
    assert not np.isin(picks2.cpu().numpy(), ex).any()
    assert cal.cal_device(_dev(rows[:9]), _dev(lab), _dev(p_pool[:9]), _dev(p_lab), 50, k_nn=3, exclude=[0])[0].numel() == 8

    # the sampler's device route equals its host route
    class Learner(object):
        X_training = lab

        def predict_proba(self, X):
            return p_lab if len(X) == M else p_pool
    idx, inst = cal.cal_sampling(Learner(), _dev(rows), n_instances=25, k_nn=K)
    assert np.array_equal(idx, want) and torch.equal(inst, _dev(rows)[torch.from_numpy(idx).cuda()])


def test_bagging_cal_indexed(gpu):
    from a_link_amd import cal, committee, siamese
    rng = np.random.RandomState(2)
    D, P, G, N = 64, 40, 7, 240
    L, R = rng.randn(P, D).astype(np.float32), rng.randn(G, D).astype(np.float32)
    li, ri = rng.randint(0, P, N).astype(np.int32), rng.randint(0, G, N).astype(np.int32)
    lab = rng.permutation(N)[:30]
    bag = committee.Bagging([siamese.SiameseNetwork((D,), "c%d" % m, 0.1, seed=90 + m) for m in range(2)], [])
    dL, dR, dli, dri = _dev(L), _dev(R), _dev(li), _dev(ri)
    picks, info = bag.cal_indexed(dL, dR, dli, dri, lab, 20, k_nn=6)
    picks = picks.cpu().numpy()
    assert len(picks) == 20 and len(set(picks.tolist())) == 20 and not np.isin(picks, lab).any()
    probs = bag.predict_indexed(dL, dR, dli, dri).cpu().numpy()
    idx = info["idx"].cpu().numpy()
    ref = (dL, dR, dli[torch.from_numpy(lab).cuda()], dri[torch.from_numpy(lab).cuda()])
    assert np.array_equal(idx, cal.knn_rect_device((dL, dR, dli, dri), ref, 6)[0].cpu().numpy()) and (info["found"] == 6).all()
    want = cal.cal_scores(probs, probs[lab], idx)
    got = info["scores"].cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want) <= score_tolerance(probs, probs[lab], idx, want)).all()
    masked = got.astype(np.float64)
    masked[lab] = -np.inf
    assert np.array_equal(picks, np.argsort(-masked, kind="stable")[:20])
    with pytest.raises(ValueError, match="one feature space"):
        bag.cal_indexed([dL] * 2, [dR] * 2, dli, dri, lab, 5)
    with pytest.raises(ValueError, match="at least one labelled pair"):
        bag.cal_indexed(dL, dR, dli, dri, [], 5)


def test_python_refusals(gpu):
    from a_link_amd import cal
    X = _dev(np.random.RandomState(3).randn(50, 8).astype(np.float32))
    Y = X[:20].contiguous()
    ind = _dev(np.arange(4, dtype=np.int32))
    with pytest.raises(ValueError, match="CUDA"):
        cal.knn_rect_device(X.cpu(), Y, 4)
    with pytest.raises(ValueError, match="float32"):
        cal.knn_rect_device(X, Y.double(), 4)
    for bad in (0, -1, 1.5, 33):
        with pytest.raises(ValueError, match="k = "):
            cal.knn_rect_device(X, Y, bad)
    with pytest.raises(ValueError, match="both"):
        cal.knn_rect_device(X, (Y, Y, ind, ind), 2)
    with pytest.raises(ValueError, match="both"):
        cal.knn_rect_device((X, X, ind, ind), Y, 2)
    with pytest.raises(ValueError, match="D = 5"):
        cal.knn_rect_device(X, Y[:, :5].contiguous(), 2)
    with pytest.raises(ValueError, match="empty"):
        cal.knn_rect_device(X, Y[:0], 2)
    with pytest.raises(ValueError, match="outside its table"):
        cal.knn_rect_device((X, X, ind, ind), (Y, Y, ind + 17, ind), 2)
    p, q = torch.full((50, 2), 0.5, device="cuda"), torch.full((20, 2), 0.5, device="cuda")
    idx = torch.zeros((50, 3), dtype=torch.int32, device="cuda")
    for bad in (dict(p_pool=p.cpu()), dict(p_pool=p.double()), dict(p_labelled=torch.full((20, 3), 0.5, device="cuda")),
                dict(p_pool=torch.full((50, 33), 0.5, device="cuda"), p_labelled=torch.full((20, 33), 0.5, device="cuda")),
                dict(idx=idx.long()), dict(idx=idx[:49]), dict(idx=torch.zeros((50, 33), dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError, match="p_pool|p_labelled|idx"):
            cal.cal_scores_device(**dict(dict(p_pool=p, p_labelled=q, idx=idx), **bad))
    with pytest.raises(ValueError, match="n_instances"):
        cal.cal_device(X, Y, p, q, 0)
    with pytest.raises(ValueError, match="labelled"):
        cal.cal_device(X, Y, p, q, 2, exclude=[50])


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    x, c = torch.zeros((8, 4), device="cuda"), torch.zeros((5, 4), device="cuda")
    ind = torch.zeros(8, dtype=torch.int32, device="cuda")
    outs = {"idx": torch.full((8, 3), -7, dtype=torch.int32, device="cuda"), "d2": torch.full((8, 3), -7.0, device="cuda"),
            "found": torch.full((8,), -7, dtype=torch.int32, device="cuda"), "score": torch.full((8,), -7.0, device="cuda")}
    size = lib.alink_knn_rect_scratch_bytes
    assert size(8, 5, 4, 33) == 0 and size(0, 5, 4, 3) == 0 and size(8, 0, 4, 3) == 0 and size(8, 2 ** 31, 4, 3) == 0 and size(8, 5, 8193, 3) == 0
    assert size(8, 5, 4, 3) == 512 and size(65, 1, 1, 1) == 768          # a function of the sizes: the two norm vectors, each 256-aligned
    scratch = torch.empty(size(8, 5, 4, 3) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(qx=x, qr=None, qli=None, qri=None, N=8, cx=c, cr=None, cli=None, cri=None, M=5, D=4, K=3, idx=outs["idx"], scratch_ptr=sp,
             full=True):
        o = [outs[k] if full else None for k in ("d2", "found")]
        return lib.alink_knn_rect(gpu.ptr(qx), gpu.ptr(qr), gpu.ptr(qli), gpu.ptr(qri), N, gpu.ptr(cx), gpu.ptr(cr), gpu.ptr(cli), gpu.ptr(cri),
                                  M, D, K, gpu.ptr(idx), gpu.ptr(o[0]), gpu.ptr(o[1]), C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(qx=None), "NULL"), (dict(cx=None), "NULL"), (dict(idx=None), "NULL"), (dict(scratch_ptr=0), "NULL"),
                     (dict(qli=ind, cli=ind, cr=c, cri=ind), "pair form"), (dict(qli=ind, qr=x, cli=ind, cr=c, cri=ind), "pair form"),
                     (dict(qli=ind, qr=x, qri=ind, cli=ind), "pair form"), (dict(qli=ind, qr=x, qri=ind, cli=ind, cri=ind), "pair form"),
                     (dict(qli=ind, qr=x, qri=ind), "mixed forms"), (dict(cli=ind, cr=c, cri=ind), "mixed forms"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(M=0), "M=0"), (dict(M=2 ** 31), "M=2147483648"),
                     (dict(D=0), "D=0"), (dict(D=8193), "D=8193"), (dict(K=0), "K=0"), (dict(K=33), "K=33"),
                     (dict(scratch_ptr=sp + 4), "aligned")):
        assert call(**kw) == -1, kw                                           # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    p, q = torch.full((8, 2), 0.5, device="cuda"), torch.full((5, 2), 0.5, device="cuda")
    lists = torch.zeros((8, 3), dtype=torch.int32, device="cuda")

    def score(p_=p, q_=q, Cn=2, idx=lists, N=8, M=5, K=3, out=outs["score"]):
        return lib.alink_cal_score(gpu.ptr(p_), gpu.ptr(q_), Cn, gpu.ptr(idx), N, M, K, gpu.ptr(out), st)
    for kw, text in ((dict(p_=None), "NULL"), (dict(q_=None), "NULL"), (dict(idx=None), "NULL"), (dict(out=None), "NULL"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(M=0), "M=0"), (dict(M=2 ** 31), "M=2147483648"),
                     (dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(Cn=0), "C=0"), (dict(Cn=33), "C=33")):
        assert score(**kw) == -1, kw
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(K=0), "alink_knn_rect")
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs.values())               # a refused call launches nothing
    assert call(full=False) == 0                                              # every output but dev_idx may be NULL
    torch.cuda.synchronize()
    assert outs["idx"].cpu().tolist() == [[0, 1, 2]] * 8
    assert bool((outs["d2"] == -7.0).all()) and bool((outs["found"] == -7).all())
    assert call() == 0 and call(M=2) == 0
    torch.cuda.synchronize()
    assert outs["found"].cpu().tolist() == [2] * 8 and outs["idx"].cpu().tolist() == [[0, 1, -1]] * 8
    assert bool(torch.isnan(outs["d2"][:, 2]).all()) and bool((outs["d2"][:, :2] == 0).all())
    # an index past the references is skipped, never read through: [0, 9, -1] scores as [0]
    lists[:, 1], lists[:, 2] = 9, -1
    q[0] = torch.tensor([0.25, 0.75])
    assert score() == 0
    torch.cuda.synchronize()
    want = 0.25 * (np.log(0.25) - np.log(0.5)) + 0.75 * (np.log(0.75) - np.log(0.5))
    assert np.allclose(outs["score"].cpu().numpy(), want, rtol=2.0 ** -23, atol=0)
