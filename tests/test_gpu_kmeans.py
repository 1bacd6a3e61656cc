"""GPU: Lloyd's k-means on device (alink_kmeans, kmeans.hip; a-link_amd/cluster.py) — bit equality with the host rule
(cluster.kmeans) on inputs that admit no rounding, T iterations against T chained calls, a row's independence of the pool around
it, the pair form against the row form, real-valued rows within the float32 bound of a D-term chain, NaN rows, non-finite centres,
exhausted seeding, the two strategies and their Bagging forms, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_cluster_host import SHAPES as MIXTURES, duplicate_pool, mixture

pytestmark = pytest.mark.gpu

KEYS = ("centres", "assign", "d2", "inertia", "changed", "counts", "wsum", "nearest")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_dev(rows):
    return tuple(_dev(a) for a in rows) if isinstance(rows, tuple) else _dev(rows)


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _run(rows, centres, T, weights=None):
    from a_link_amd import cluster
    out = cluster.kmeans_device(_rows_dev(rows), len(centres), iters=T, weights=None if weights is None else _dev(np.asarray(weights, np.float32)),
                                centres=_dev(np.asarray(centres, np.float32)))
    assert out["assign"].dtype == torch.int32 and out["d2"].dtype == torch.float32 and out["inertia"].dtype == torch.float64
    assert out["changed"].dtype == torch.int32 and out["counts"].dtype == torch.int32 and out["wsum"].dtype == torch.float64
    assert out["nearest"].dtype == torch.int32 and out["centres"].dtype == torch.float32 and all(v.is_cuda for v in out.values())
    assert out["inertia"].shape == (T + 1,) and out["changed"].shape == (T + 1,)
    return _host(out)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b, keys=KEYS):
    """two device results equal bit for bit -> the first key that differs, or None"""
    for k in keys:
        if a[k].dtype != b[k].dtype or not np.array_equal(_bits(a[k]), _bits(b[k])):
            return k
    return None


def _equals_host(got, want, keys=KEYS):
    """a device result against cluster.kmeans: integers equal, floats equal as values with NaN where the host has NaN (the host
    keeps d2 in float64: an exact value is the same number in both) -> the first key that differs, or None"""
    for k in keys:
        g, w = got[k], want[k]
        if g.shape != w.shape:
            return k
        if g.dtype.kind == "f":
            g, w = g.astype(np.float64), w.astype(np.float64)
            if not (np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(g)], w[~np.isnan(w)])):
                return k
        elif not np.array_equal(g, w.astype(g.dtype)):
            return k
    return None


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


# (N, D, K).  The assignment's tiles: 128 rows a workgroup (32 a wave), 128 centres a tile in blocks of 32, 32 columns a chunk; the
# light pass takes chunks of 8 rows (16 beyond 16,384 rows), the update's scan 256 rows a step and 256 columns a wave.  The first
# eight leave every tile ragged (one row, K > N, D off 4, D above 256 and 512, N beyond one sweep of the capped grid); the rest
# sit one below, on and one above each tile size.
INT_SHAPES = [(1, 5, 1), (4, 6, 10), (777, 40, 64), (1031, 512, 33), (300, 7, 300), (130, 600, 3), (16391, 12, 130), (40000, 128, 64),
              (127, 31, 127), (128, 32, 128), (129, 33, 129), (255, 63, 31), (256, 64, 32), (257, 65, 33), (31, 255, 7), (33, 257, 9)]


def _int_case(N, D, K, seed=0):
    rng = np.random.RandomState(300 + N + seed)
    X = rng.randint(-8, 9, (N, D)).astype(np.float32)
    Cn = rng.randint(-8, 9, (K, D)).astype(np.float32)
    if K > 2:                                              # duplicate centres: ties that must go to the lower index
        Cn[K - 1] = Cn[0]
        Cn[K // 2] = Cn[1]
    return rng, X, Cn


@pytest.mark.parametrize("N,D,K", INT_SHAPES)
def test_assignment_bit_equal_to_the_host_rule(gpu, N, D, K):
    """features and centres in [-8, 8]: every product, score, d2 and float64 sum is an integer far below 2^24 — exact in any
    order, so the device must give the host's outputs bit for bit"""
    from a_link_amd import cluster
    rng, X, Cn = _int_case(N, D, K)
    for w in (None, rng.randint(0, 4, N).astype(np.float32)):
        want = cluster.kmeans(X, Cn, 0, weights=w)
        got = _run(X, Cn, 0, weights=w)
        assert _equals_host(got, want) is None, _equals_host(got, want)
        if K > 2:
            assert want["counts"][K - 1] == 0 and want["nearest"][K - 1] == -1
        assert np.array_equal(got["centres"], Cn) and got["changed"][0] == N


@pytest.mark.parametrize("N,D,K", [(4, 6, 10), (777, 40, 64), (1031, 512, 33), (300, 7, 300), (130, 600, 3), (16391, 12, 130),
                                   (129, 257, 5), (2000, 255, 9), (515, 256, 2)])
def test_one_iteration_bit_equal_centres(gpu, N, D, K):
    """one update on integer rows, with and without small-integer weights (zeros among them): both sides hold the exact float64
    sums, divide once and round once — the centres are equal bit for bit; a cluster without rows or weight keeps its centre"""
    from a_link_amd import cluster
    rng, X, Cn = _int_case(N, D, K, seed=1)
    for w in (None, rng.randint(0, 4, N).astype(np.float32)):
        want = cluster.kmeans(X, Cn, 1, weights=w)
        got = _run(X, Cn, 1, weights=w)
        assert np.array_equal(_bits(got["centres"]), _bits(want["centres"]))
        assert got["inertia"][0] == want["inertia"][0] and got["changed"][0] == N
        first = cluster.kmeans(X, Cn, 0, weights=w)
        kept = first["wsum"] == 0
        assert np.array_equal(got["centres"][kept], Cn[kept])
        if K > 2:
            assert kept[K - 1]


def _blobs(B, D, seed):
    """B blobs of 16 integer rows, blob b around 64 e_b with jitter in {-1, 0, 1}, shuffled; one row of each blob as its centre"""
    rng = np.random.RandomState(seed)
    base = np.zeros((B, D))
    base[np.arange(B), np.arange(B) % D] = 64
    blob = np.repeat(np.arange(B), 16)
    X = base[blob] + rng.randint(-1, 2, (16 * B, D))
    perm = rng.permutation(16 * B)
    X, blob = X[perm].astype(np.float32), blob[perm]
    C0 = np.stack([X[np.flatnonzero(blob == b)[0]] for b in range(B)])
    return X, C0, blob


@pytest.mark.parametrize("B,D", [(12, 40), (33, 512)])
def test_several_iterations_bit_equal_on_integer_blobs(gpu, B, D):
    """the means of 16 integer rows are multiples of 1/16, so every later product, score and distance stays exact as long as
    16 |x||c| and 256 |c|^2 stay below 2^24 (asserted on the host first): T = 3 is bit-equal to the host throughout"""
    from a_link_amd import cluster
    X, C0, blob = _blobs(B, D, 60 + B)
    T = 3
    X64 = np.abs(X.astype(np.float64))
    for t in range(T + 1):
        Ct = np.abs(cluster.kmeans(X, C0, t)["centres"].astype(np.float64))
        assert np.array_equal(Ct * 16, np.round(Ct * 16))
        assert 16 * (X64 @ Ct.T).max() < 2 ** 24 and 256 * (Ct * Ct).sum(axis=1).max() < 2 ** 24
        assert 256 * ((X64[:, None, :] + Ct[None, :, :]) ** 2).sum(axis=2).max() < 2 ** 24       # every d2 and score too
    want = cluster.kmeans(X, C0, T)
    assert want["changed"].tolist() == [16 * B, 0, 0, 0] and np.array_equal(want["assign"], blob) and (want["counts"] == 16).all()
    got = _run(X, C0, T)
    assert _equals_host(got, want) is None, _equals_host(got, want)


@pytest.mark.parametrize("case", [0, 2])
def test_T_iterations_equal_T_chained_calls(gpu, case):
    """real-valued rows, T = 6 (the (777, 7, 5) mixture keeps reassigning that long): one call equals six calls of one iteration
    each fed the centres of the one before, bit for bit — the launches of one call hand on exactly what a finished call holds"""
    N, D, K = MIXTURES[case]
    X, C0 = mixture(N, D, K, 50 + case)
    w = np.random.RandomState(case).uniform(0.5, 2.0, N).astype(np.float32)
    T = 6
    whole = _run(X, C0, T, weights=w)
    Ct, step = C0, None
    for t in range(T):
        step = _run(X, Ct, 1, weights=w)
        assert _bits(step["inertia"])[0] == _bits(whole["inertia"])[t] and _bits(step["inertia"])[1] == _bits(whole["inertia"])[t + 1]
        assert step["changed"][1] == whole["changed"][t + 1]
        Ct = step["centres"]
    assert _same(step, whole, ("centres", "assign", "d2", "counts", "wsum", "nearest")) is None
    if case == 2:
        assert (whole["changed"] > 0).all()


def test_a_rows_result_does_not_depend_on_the_pool_around_it(gpu):
    from a_link_amd import cluster
    for D in (40, 7, 512):
        N, K = 1003, 16
        X, C0 = mixture(N, D, K, 77)
        full = _run(X, C0, 0)
        head = _run(X[:200], C0, 0)
        assert np.array_equal(head["assign"], full["assign"][:200]) and np.array_equal(_bits(head["d2"]), _bits(full["d2"][:200]))
        # the same table 4 bytes off the 16-byte alignment (the scalar loads)
        buf = torch.empty(N * D + 1, device="cuda")
        buf[1:] = _dev(X).reshape(-1)
        xo = buf[1:].view(N, D)
        assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
        off = _host(cluster.kmeans_device(xo, K, iters=3, centres=_dev(C0)))
        assert _same(off, _run(X, C0, 3)) is None
        assert _same(_run(X, C0, 3), _run(X, C0, 3)) is None          # two runs of a call


@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D):
    from a_link_amd import cluster
    rng = np.random.RandomState(D)
    P, G, N, K = 60, 9, 700, 12
    li, ri = rng.randint(0, P, N).astype(np.int32), rng.randint(0, G, N).astype(np.int32)
    w = rng.randint(0, 4, N).astype(np.float32)
    for integer in (True, False):
        L = rng.randint(-4, 5, (P, D)).astype(np.float32) if integer else _unit(rng.randn(P, D))
        R = rng.randint(-4, 5, (G, D)).astype(np.float32) if integer else _unit(rng.randn(G, D))
        X = np.abs(L[li] - R[ri])                           # one rounded subtraction: the bits the on-the-fly row holds
        C0 = X[rng.choice(N, K, replace=False)].copy()
        for T in (0, 3):
            pair, row = _run((L, R, li, ri), C0, T, weights=w), _run(X, C0, T, weights=w)
            assert _same(pair, row) is None, (_same(pair, row), integer, T)
        if integer:
            want = cluster.kmeans(X, C0, 0, weights=w)
            assert _equals_host(_run((L, R, li, ri), C0, 0, weights=w), want) is None
            one = cluster.kmeans(X, C0, 1, weights=w)
            assert np.array_equal(_bits(_run((L, R, li, ri), C0, 1, weights=w)["centres"]), _bits(one["centres"]))


def _real_cases():
    rng = np.random.RandomState(5)
    a, b = _unit(rng.randn(50, 64)), _unit(rng.randn(12, 64))
    li, ri = rng.randint(0, 50, 900).astype(np.int32), rng.randint(0, 12, 900).astype(np.int32)
    X = np.abs(a[li] - b[ri])
    yield "unit pairs", (a, b, li, ri), X, X[:10].copy(), None
    for case, (N, D, K) in enumerate(MIXTURES):
        X, C0 = mixture(N, D, K, 50 + case)
        yield "mixture %d" % case, X, X, C0, np.random.RandomState(case).uniform(0.5, 2.0, N).astype(np.float32) if case % 2 else None


def test_real_valued_rows_within_the_float32_bound(gpu):
    """g = (D + 8) 2^-24 bounds a D-term float32 chain; E(n, j) = g (|c_j|^2 + 2 |x_n| |c_j|) bounds the error of score(n, j).
    In float64 on the device's final centres: d2(n, a_n) <= min_j d2(n, j) + E(n, a_n) + E(n, j*); each centre within one float32
    ulp of the float64 weighted mean of the rows the device assigned to it in the pass before; inertia non-increasing within g"""
    T = 6
    for name, rows, X, C0, w in _real_cases():
        N, D = X.shape
        g = (D + 8) * 2.0 ** -24
        got, before = _run(rows, C0, T, weights=w), _run(rows, C0, T - 1, weights=w)
        X64, Cf = X.astype(np.float64), got["centres"].astype(np.float64)
        d2 = np.stack([((X64 - c) ** 2).sum(axis=1) for c in Cf], axis=1)
        a = got["assign"]
        assert (a >= 0).all()
        xn, cn = np.sqrt((X64 * X64).sum(axis=1)), np.sqrt((Cf * Cf).sum(axis=1))
        E = g * (cn[None, :] ** 2 + 2 * xn[:, None] * cn[None, :])
        js = d2.argmin(axis=1)
        rows_ = np.arange(N)
        excess = d2[rows_, a] - d2[rows_, js]
        room = E[rows_, a] + E[rows_, js]
        print("%s: largest excess of the assigned distance %.3e, %.3g of its bound; %d rows off the float64 argmin" %
              (name, excess.max(), (excess / room).max(), int((a != js).sum())))
        assert (excess <= room).all()
        own = ((X64 - Cf[a]) ** 2).sum(axis=1)
        assert np.abs(got["d2"] - own).max() <= g * own.max() + 1e-30
        wd = np.ones(N) if w is None else w.astype(np.float64)
        worst = 0.0
        for j in range(len(Cf)):
            m = before["assign"] == j
            assert m.any()
            mean = (wd[m, None] * X64[m]).sum(axis=0) / wd[m].sum()
            ulp = np.spacing(np.abs(got["centres"][j]))
            assert (np.abs(Cf[j] - mean) <= ulp).all()
            worst = max(worst, (np.abs(Cf[j] - mean) / ulp).max())
        print("%s: centres within %.3f ulp of the float64 mean" % (name, worst))
        assert (got["inertia"][1:] <= got["inertia"][:-1] * (1 + g)).all()
        assert np.array_equal(_bits(got["inertia"][:T]), _bits(before["inertia"]))


def test_nan_rows_and_non_finite_centres(gpu):
    from a_link_amd import cluster
    X = np.array([[0., 0.], [np.nan, 0.], [4., 0.], [0., 0.]], np.float32)
    Cn = np.array([[1., 0.], [np.inf, 0.], [5., 0.]], np.float32)
    for T in (0, 1, 2):
        want = cluster.kmeans(X, Cn, T)
        got = _run(X, Cn, T)
        assert _equals_host(got, want) is None, (T, _equals_host(got, want))
    assert got["assign"].tolist() == [0, -1, 2, 0] and got["nearest"].tolist() == [0, -1, 2]
    # a ragged pool with NaN rows and -inf / NaN / +inf centres among integer ones, with zero weights
    rng, X, Cn = _int_case(1500, 37, 70)
    X[rng.choice(1500, 40, replace=False), rng.randint(0, 37, 40)] = np.nan
    Cn[3, 5], Cn[40, 36], Cn[69, 0] = np.inf, np.nan, -np.inf
    w = rng.randint(0, 3, 1500).astype(np.float32)
    want = cluster.kmeans(X, Cn, 0, weights=w)
    got = _run(X, Cn, 0, weights=w)
    assert _equals_host(got, want) is None, _equals_host(got, want)
    assert (got["assign"] == -1).sum() == 40 and got["counts"][[3, 40, 69]].tolist() == [0, 0, 0]
    one = _run(X, Cn, 1, weights=w)
    assert np.array_equal(_bits(one["centres"]), _bits(cluster.kmeans(X, Cn, 1, weights=w)["centres"]))
    assert np.array_equal(_bits(one["centres"][[3, 40, 69]]), _bits(Cn[[3, 40, 69]]))


def test_exhausted_seeding_leaves_empty_clusters(gpu):
    """fewer distinct rows than clusters: the seeding's -1 picks become centres of +inf, which stay empty — as on the host"""
    from a_link_amd import badge, cluster
    rng = np.random.RandomState(8)
    base = rng.randint(-8, 9, (5, 6)).astype(np.float32)
    X = base[rng.randint(0, 5, 60)]
    for N, K in ((60, 8), (4, 10)):
        Xn = X[:N]
        u = rng.random_sample(min(K, N))
        seeds, _ = badge.kmeans_pp(Xn, min(K, N), u)
        Cn = np.full((K, 6), np.inf, np.float32)
        Cn[:len(seeds)][seeds >= 0] = Xn[seeds[seeds >= 0]]
        want = cluster.kmeans(Xn, Cn, 2)
        got = _host(cluster.kmeans_device(_dev(Xn), K, iters=2, uniforms=u))
        assert _equals_host(got, want) is None, _equals_host(got, want)
        distinct = len({r.tobytes() for r in Xn})
        assert (got["nearest"] >= 0).sum() == distinct and (got["nearest"] == -1).sum() == K - distinct
        assert (got["d2"] == 0).all() and got["inertia"].tolist() == [0.0] * 3


def test_kmeans_sampling_device_on_a_pool_of_duplicates(gpu):
    """40 distinct pairs, each ten times in the pool: a batch of 40 takes every pair once"""
    from a_link_amd import cluster
    D = 64
    rng = np.random.RandomState(13)
    L, R = _unit(rng.randn(40, D)), _unit(rng.randn(40, D))
    perm = rng.permutation(400)
    li = np.repeat(np.arange(40, dtype=np.int32), 10)[perm]
    idx, info = cluster.kmeans_sampling_device((_dev(L), _dev(R), _dev(li), _dev(li.copy())), 40, seed=1)
    idx = idx.cpu().numpy()
    assert idx.shape == (40,) and (idx >= 0).all() and len({int(li[i]) for i in idx}) == 40
    assert torch.equal(info["nearest"].cpu(), torch.from_numpy(idx)) and (info["counts"].cpu().numpy() == 10).all()
    Lh, Rh, _ = duplicate_pool()
    idx, _ = cluster.kmeans_sampling(None, [_dev(Lh), _dev(Rh)], n_instances=40, random_state=3)     # the sampler's device route
    assert idx.shape == (40,) and len({Lh[i].tobytes() for i in idx}) == 40
    idx, _ = cluster.kmeans_sampling_device(_dev(Lh), 1000, seed=2)                                  # K is clipped to N
    assert idx.shape == (400,) and (idx.cpu().numpy() >= 0).sum() == 40


class _Clf(object):
    def __init__(self, proba):
        self.proba = proba

    def predict_proba(self, X):
        return self.proba


def test_diverse_minibatch_device_stays_in_the_top_and_equals_the_host_route(gpu):
    from a_link_amd import cluster
    rng = np.random.RandomState(21)
    N, D = 3000, 12
    L, R = rng.randint(-8, 9, (N, D)).astype(np.float32), rng.randint(-8, 9, (N, D)).astype(np.float32)
    p = rng.uniform(0.5, 1.0, N)
    clf = _Clf(np.stack([p, 1 - p], axis=1))
    utility = (1 - p).astype(np.float32)
    ar = np.arange(N, dtype=np.int32)
    for k, beta in ((8, 5), (16, 10), (5, 1)):
        top = np.argsort(-utility, kind="stable")[:beta * k]
        want, _ = cluster.diverse_minibatch_sampling(clf, [L, R], n_instances=k, beta=beta, random_state=6, iters=3)
        for rows in (_dev(np.abs(L - R)), (_dev(L), _dev(R), _dev(ar), _dev(ar))):
            idx, info = cluster.diverse_minibatch_device(rows, _dev(utility), k, beta=beta, iters=3, seed=6)
            idx = idx.cpu().numpy()
            assert idx.shape == (k,) and set(idx[idx >= 0].tolist()) <= set(top.tolist())
            assert np.array_equal(info["top"].cpu().numpy(), top) and info["assign"].shape == (beta * k,)
            assert np.array_equal(idx[idx >= 0], want)
        got, inst = cluster.diverse_minibatch_sampling(clf, [_dev(L), _dev(R)], n_instances=k, beta=beta, random_state=6, iters=3)
        assert np.array_equal(got, want) and torch.equal(inst[0], _dev(L)[torch.from_numpy(got).cuda()]) and torch.equal(inst[1], inst[0])


def _committee(D, members=3):
    from a_link_amd import committee, siamese
    nets = []
    for m in range(members):
        net = siamese.SiameseNetwork((D,), "c%d" % m, 0.1, seed=80 + m)
        ws = net.siamese_net.get_weights()
        ws[4] = ws[4] * np.float32(40.0)                                        # probabilities spread over (0, 1)
        net.siamese_net.set_weights(ws)
        nets.append(net)
    return committee.Bagging(nets, [])


def test_the_two_bagging_methods_equal_the_module_functions(gpu):
    from a_link_amd import cluster, uncertainty
    D, n_pairs, k = 64, 500, 6
    rng = np.random.RandomState(9)
    L, R = _dev(_unit(rng.randn(40, D))), _dev(_unit(rng.randn(9, D)))
    li, ri = _dev(rng.randint(0, 40, n_pairs).astype(np.int32)), _dev(rng.randint(0, 9, n_pairs).astype(np.int32))
    bag = _committee(D)
    u = rng.random_sample(k)
    got = bag.kmeans_sampling_indexed(L, R, li, ri, k, iters=4, uniforms=u)
    want = cluster.kmeans_sampling_device((L, R, li, ri), k, iters=4, uniforms=u)
    assert torch.equal(got[0], want[0]) and _same(_host(got[1]), _host(want[1])) is None
    for kind in ("entropy", "uncertainty"):
        utility = uncertainty.score_device(bag.predict_indexed(L, R, li, ri), kind)
        got = bag.diverse_minibatch_indexed(L, R, li, ri, k, kind=kind, beta=7, iters=4, uniforms=u)
        want = cluster.diverse_minibatch_device((L, R, li, ri), utility, k, beta=7, iters=4, uniforms=u)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1]["top"], want[1]["top"])
        assert _same(_host(got[1]), _host(want[1])) is None and got[1]["assign"].numel() == 42
    with pytest.raises(ValueError, match="one feature space"):
        bag.kmeans_sampling_indexed([L] * 3, [R] * 3, li, ri, k)
    with pytest.raises(ValueError, match="one feature space"):
        bag.diverse_minibatch_indexed([L] * 3, [R] * 3, li, ri, k)
    with pytest.raises(ValueError, match="unknown utility kind"):
        bag.diverse_minibatch_indexed(L, R, li, ri, k, kind="margin")


def test_python_refusals(gpu):
    from a_link_amd import cluster
    rng = np.random.RandomState(3)
    X = _dev(rng.randn(50, 8).astype(np.float32))
    Cn = X[:4].clone()
    run = cluster.kmeans_device
    with pytest.raises(ValueError, match="CUDA"):
        run(X.cpu(), 4)
    with pytest.raises(ValueError, match="float32"):
        run(X.double(), 4)
    with pytest.raises(ValueError, match="n_clusters"):
        run(X, 0)
    with pytest.raises(ValueError, match="n_clusters"):
        run(X, 8193)
    with pytest.raises(ValueError, match="iters"):
        run(X, 4, iters=-1)
    with pytest.raises(ValueError, match="weights"):
        run(X, 4, weights=torch.ones(49, device="cuda"))
    with pytest.raises(ValueError, match="weights"):
        run(X, 4, weights=torch.ones(50, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="centres"):
        run(X, 4, centres=Cn.cpu())
    with pytest.raises(ValueError, match="centres has D = 7"):
        run(X, 4, centres=Cn[:, :7])
    with pytest.raises(ValueError, match="uniforms"):
        run(X, 4, uniforms=[0.5])
    with pytest.raises(ValueError, match="D = 8200"):
        run(torch.zeros((2, 8200), device="cuda"), 1)
    li = _dev(np.arange(4, dtype=np.int32))
    with pytest.raises(ValueError, match="outside its table"):
        run((X, X, li + 47, li), 2)
    for fn in (lambda n: cluster.kmeans_sampling_device(X, n), lambda n: cluster.diverse_minibatch_device(X, X[:, 0].contiguous(), n)):
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match="n_instances"):
                fn(bad)
    with pytest.raises(ValueError, match="beta"):
        cluster.diverse_minibatch_device(X, X[:, 0].contiguous(), 3, beta=0)
    with pytest.raises(ValueError, match="utility"):
        cluster.diverse_minibatch_device(X, X[:9, 0].contiguous(), 3)


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    x = torch.zeros((8, 4), device="cuda")
    ind = torch.zeros(8, dtype=torch.int32, device="cuda")
    cen = torch.full((4, 4), -7.0, device="cuda")
    outs = {"assign": torch.full((8,), -7, dtype=torch.int32, device="cuda"), "d2": torch.full((8,), -7.0, device="cuda"),
            "inertia": torch.full((3,), -7.0, dtype=torch.float64, device="cuda"), "changed": torch.full((3,), -7, dtype=torch.int32, device="cuda"),
            "counts": torch.full((4,), -7, dtype=torch.int32, device="cuda"), "wsum": torch.full((4,), -7.0, dtype=torch.float64, device="cuda"),
            "nearest": torch.full((4,), -7, dtype=torch.int32, device="cuda")}
    scratch = torch.empty(lib.alink_kmeans_scratch_bytes(8, 4, 4) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(x_=x, r=None, li=None, ri=None, N=8, D=4, w=None, cen_=cen, K=4, iters=2, assign=outs["assign"], scratch_ptr=sp, full=True):
        o = [outs[k] if full else None for k in ("d2", "inertia", "changed", "counts", "wsum", "nearest")]
        return lib.alink_kmeans(gpu.ptr(x_), gpu.ptr(r), gpu.ptr(li), gpu.ptr(ri), N, D, gpu.ptr(w), gpu.ptr(cen_), K, iters, gpu.ptr(assign),
                                gpu.ptr(o[0]), gpu.ptr(o[1]), gpu.ptr(o[2]), gpu.ptr(o[3]), gpu.ptr(o[4]), gpu.ptr(o[5]), C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(x_=None), "NULL"), (dict(cen_=None), "NULL"), (dict(assign=None), "NULL"), (dict(scratch_ptr=0), "NULL"),
                     (dict(li=ind), "pair form"), (dict(li=ind, r=x), "pair form"), (dict(li=ind, ri=ind), "pair form"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(D=0), "D=0"), (dict(D=8193), "D=8193"),
                     (dict(K=0), "K=0"), (dict(K=8193), "K=8193"), (dict(iters=-1), "iters=-1"), (dict(scratch_ptr=sp + 4), "aligned")):
        assert call(**kw) == -1, kw                                           # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(K=0), "alink_kmeans")
    torch.cuda.synchronize()
    assert bool((cen == -7.0).all()) and all(bool((v == -7).all()) for v in outs.values())      # a refused call launches nothing
    cen.copy_(torch.tensor([[0., 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [2, 2, 2, 2]]))
    assert call(full=False) == 0                                              # every output but the two required ones may be NULL
    torch.cuda.synchronize()
    assert outs["assign"].cpu().tolist() == [0] * 8 and bool((outs["d2"] == -7.0).all()) and bool((outs["nearest"] == -7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert outs["counts"].cpu().tolist() == [8, 0, 0, 0] and outs["nearest"].cpu().tolist() == [0, -1, -1, -1]
    assert outs["changed"].cpu().tolist() == [8, 0, 0] and outs["inertia"].cpu().tolist() == [0.0] * 3 and outs["wsum"].cpu().tolist() == [8.0, 0, 0, 0]
