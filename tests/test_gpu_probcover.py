"""GPU: the delta-ball graph, the purity outputs and the greedy maximum coverage on device (alink_ball_count, alink_ball_fill,
alink_max_coverage, probcover.hip; a-link_amd/probcover.py) — bit equality with the host rule on small-integer rows around every
size the kernel has, a pool where every ball is the pool, the pair form against the row form, rows that are not eligible,
real-valued rows within the float32 band of a D-term chain and symmetric bit for bit, the greedy against the host on random and
hand-built graphs, ProbCover end to end against the host, its Bagging and ActiveLearner forms, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_knn import INT_SHAPES, _pair_of
from test_probcover_host import (BAND_SHARE, QUANTILES, REAL_SHAPES, delta_of, dense, graph_within_float32_bound, pair_d2,
                                 quantile_radius2, random_csr, real_rows)
from test_typiclust_host import blobs, int_rows, random_groups

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_dev(rows):
    return tuple(_dev(a) for a in rows) if isinstance(rows, tuple) else _dev(rows)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _run(rows, r2, groups=None):
    """count (with the purity outputs where there are groups) and fill -> (deg, offsets, nbr[, t_other, j_other]) as NumPy arrays.
    ball_graph_device asserts the fill's mismatch count to be 0."""
    from a_link_amd import probcover
    rows = rows if isinstance(rows, torch.Tensor) else _rows_dev(rows)
    g = None if groups is None else _dev(np.asarray(groups, np.int32))
    deg, t_other, j_other = probcover._ball_count(probcover._pool(rows, g, "test"), np.float32(r2), True, g is not None)
    offsets, nbr = probcover.ball_graph_device(rows, delta_of(r2), g)
    assert deg.dtype == torch.int32 and offsets.dtype == torch.int64 and nbr.dtype == torch.int32
    assert offsets.shape == (deg.shape[0] + 1,) and nbr.shape == (int(offsets[-1]),)
    out = [deg, offsets, nbr] + ([t_other, j_other] if g is not None else [])
    return tuple(t.cpu().numpy() for t in out)


def _host(X, r2, groups=None):
    from a_link_amd import probcover
    offsets, nbr = probcover.ball_graph(X, delta_of(r2), groups)
    out = [np.diff(offsets).astype(np.int32), offsets, nbr]
    if groups is not None:
        t_other, j_other = probcover.nearest_other(X, groups)
        out += [t_other.astype(np.float32), j_other]
    return tuple(out)


def _occurring_radius2(X):
    """an integer that occurs as some pair's squared distance: the median of the off-diagonal ones"""
    d2 = pair_d2(X)
    off = np.sort(d2[~np.eye(len(X), dtype=bool)])
    return float(off[len(off) // 2]), d2


# (N, D) of test_gpu_knn.INT_SHAPES: a lone row; one below / on / one above a 32-block and a 128-tile; several workgroups; D tails; D = 1
INT_ND = sorted(set((N, D) for N, D, _ in INT_SHAPES))


@pytest.mark.parametrize("N,D", INT_ND)
def test_integer_rows_bit_equal_to_the_host_rule(gpu, N, D):
    """rows in -4 .. 4: every product, norm and t is an integer far below 2^24 — exact in any order, so deg, offsets, nbr, t_other
    and j_other must equal the host's bit for bit; radius2 is a value some pair has exactly, so the strict `<` is exercised"""
    X = int_rows(N, D)
    if N == 1:
        got = _run(X, 4.0)
        assert _same_bits(got, _host(X, 4.0)) and got[2].tolist() == [0] and got[1].tolist() == [0, 1]
        return
    r2, d2 = _occurring_radius2(X)
    assert r2 == int(r2) and r2 > 0 and (d2 == r2).any()                   # pairs exactly on the radius
    got = _run(X, r2)
    want = _host(X, r2)
    assert _same_bits(got, want), [np.array_equal(a, b) for a, b in zip(got, want)]
    E = len(got[2])
    if N > 2:
        assert N < E < N * N, (N, E)
    assert _same_bits(_run(X, r2), got)                                    # two runs of a call
    g = random_groups(N, 3)
    got = _run(X, r2, g)
    want = _host(X, r2, g)
    assert _same_bits(got, want), [np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, want)]
    assert (got[0][g < 0] == 0).all() and not np.isin(got[2], np.flatnonzero(g < 0)).any()
    assert _same_bits(_run(X, r2, g), got)


def test_a_pool_of_identical_rows(gpu):
    """everything lies at distance 0: every ball is the pool"""
    for N, D in ((300, 7), (129, 32), (20, 3)):
        X = np.tile(int_rows(1, D), (N, 1))
        deg, offsets, nbr = _run(X, 0.25)
        assert (deg == N).all() and np.array_equal(offsets, np.arange(N + 1) * N)
        assert np.array_equal(nbr.reshape(N, N), np.tile(np.arange(N, dtype=np.int32), (N, 1)))


@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D):
    rng = np.random.RandomState(D)
    P, G, N = 60, 9, 300
    li, ri = rng.randint(0, P, N).astype(np.int32), rng.randint(0, G, N).astype(np.int32)
    groups = random_groups(N, 3)
    for integer in (True, False):
        L = rng.randint(-2, 3, (P, D)).astype(np.float32) if integer else rng.randn(P, D).astype(np.float32)
        R = rng.randint(-2, 3, (G, D)).astype(np.float32) if integer else rng.randn(G, D).astype(np.float32)
        X = np.abs(L[li] - R[ri])                           # one rounded subtraction: the bits the on-the-fly row holds
        r2 = _occurring_radius2(X)[0] if integer else quantile_radius2(X, 0.1)
        for g in (None, groups):
            pair, row = _run((L, R, li, ri), r2, g), _run(X, r2, g)
            assert _same_bits(pair, row), (integer, g is None)
            assert N < len(pair[2]) < N * N
            if integer:
                assert _same_bits(pair, _host(X, r2, g))
    # the same table 4 bytes off the 16-byte alignment (the scalar loads)
    X = rng.randn(N, D).astype(np.float32)
    r2 = quantile_radius2(X, 0.1)
    buf = torch.empty(N * D + 1, device="cuda")
    buf[1:] = _dev(X).reshape(-1)
    xo = buf[1:].view(N, D)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    assert _same_bits(_run(xo, r2, groups), _run(X, r2, groups))


def test_rows_that_are_not_eligible(gpu):
    """groups < 0, a NaN row and a +inf row: degree 0, in nobody's list, never covered, never picked; the others' graph as if
    those rows were absent"""
    from a_link_amd import probcover
    N, D = 200, 33
    X = int_rows(N, D)
    g = random_groups(N, 3)
    g[[5, 150]] = 1
    X[5, 7] = np.nan
    X[150, 32] = np.inf
    dead = (g < 0) | np.isin(np.arange(N), [5, 150])
    clean = np.where(dead[:, None], 0, X)
    r2, _ = _occurring_radius2(clean[~dead])
    got = _run(X, r2, g)
    want = _host(X, r2, g)
    assert _same_bits(got, want)
    deg, offsets, nbr, t_other, j_other = got
    assert (deg[dead] == 0).all() and (deg[~dead] > 0).all() and not np.isin(nbr, np.flatnonzero(dead)).any()
    assert np.isinf(t_other[dead]).all() and (j_other[dead] == -1).all() and not np.isin(j_other, np.flatnonzero(dead)).any()
    sub = _run(X[~dead], r2, g[~dead])
    back = np.flatnonzero(~dead).astype(np.int32)
    assert np.array_equal(back[sub[2]], nbr) and np.array_equal(sub[0], deg[~dead])
    k = int((~dead).sum()) + 3
    picks, info = probcover.probcover_device(_dev(X), [], k, delta=delta_of(r2), groups=_dev(g))
    hpicks, hinfo = probcover.probcover(X, [], k, delta=delta_of(r2), groups=g)
    assert np.array_equal(picks, hpicks) and info["exhausted"] and info["covered"] == 1.0 and not dead[picks].any()
    cov = info["covered_rows"].cpu().numpy()
    assert not cov[dead].any() and cov[~dead].all()
    filled, _ = probcover.probcover_device(_dev(X), [], k, delta=delta_of(r2), groups=_dev(g), fill="random", random_state=2)
    hfilled, _ = probcover.probcover(X, [], k, delta=delta_of(r2), groups=g, fill="random", random_state=2)
    assert np.array_equal(filled, hfilled) and len(filled) == k - 3 and not dead[filled].any()      # no more eligible rows than that


@pytest.mark.parametrize("N,D", REAL_SHAPES)
def test_real_valued_rows_within_the_float32_band_and_symmetric(gpu, N, D):
    """test_probcover_host.graph_within_float32_bound: no pair outside the band |d2 - radius2| <= (D + 8) 2^-24 (|x_n| + |x_j|)^2
    may differ from the float64 graph; (n, j) is an edge exactly when (j, n) is.  Measured on one MI355X: in all twelve cases no
    pair differs from the float64 graph; the band holds 0 to 9.7e-4 of the pairs."""
    X = real_rows(N, D)
    for q in QUANTILES:
        r2 = quantile_radius2(X, q)
        deg, offsets, nbr = _run(X, r2)
        fails, differ, share = graph_within_float32_bound(X, r2, offsets, nbr)
        print("%d x %d, radius2 at %g: %d pairs differ from the float64 graph; %.3g of the pairs lie in the band" % (N, D, q, differ, share))
        assert not fails, fails[:3]
        assert share <= BAND_SHARE
        A = dense(offsets, nbr)
        assert np.array_equal(A, A.T) and A.diagonal().all() and np.array_equal(deg, np.diff(offsets))
        assert N < len(nbr) < N * N


# ---- the greedy --------------------------------------------------------------------------------------------------------------
def _sparse_csr(N, seed=0, top=6):
    """random_csr without the dense matrix: few distinct degrees, so heavy ties; a row with neighbours holds itself"""
    rng = np.random.RandomState(4000 + N + seed)
    lists = []
    for u in range(N):
        d = int(rng.randint(0, top + 1))
        lists.append(np.unique(np.append(rng.randint(0, N, d), u)) if d else np.zeros(0, np.int64))
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum([len(v) for v in lists])
    return offsets, np.concatenate(lists).astype(np.int32) if offsets[-1] else np.zeros(0, np.int32)


def _greedy_both(offsets, nbr, k, seeds=(), covered=None):
    from a_link_amd import probcover
    want = probcover.max_coverage(offsets, nbr, k, seeds=seeds, covered=covered)
    got = probcover.max_coverage_device(_dev(offsets), _dev(nbr), k, seeds=list(seeds) if len(seeds) else None,
                                        covered=None if covered is None else _dev(covered))
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32 and got[2].dtype == torch.uint8
    got = tuple(t.cpu().numpy() for t in got)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), (got[0][:8], want[0][:8], got[1][:8], want[1][:8])
    return got


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000])
def test_max_coverage_equals_the_host_on_random_graphs(gpu, N):
    k = N + 3 if N <= 257 else 50                                          # the small ones past exhaustion
    offsets, nbr = random_csr(N, 1) if N <= 257 else _sparse_csr(N)
    picks, gain, covered = _greedy_both(offsets, nbr, k)
    if N <= 257:
        assert picks[-1] == -1 and gain[-1] == 0
    if N >= 63:
        assert (np.diff(gain[picks >= 0]) == 0).sum() > 3                  # ties among the picks' degrees
    again = _greedy_both(offsets, nbr, k)
    assert all(np.array_equal(a, b) for a, b in zip(again, (picks, gain, covered)))        # two runs of a call
    seeds = tuple(np.random.RandomState(N).choice(N, min(N, 5), replace=False).tolist())
    pre = np.zeros(N, np.uint8)
    pre[::3] = 1
    _greedy_both(offsets, nbr, k, seeds=seeds)
    _greedy_both(offsets, nbr, k, seeds=seeds, covered=pre)


def test_max_coverage_on_hand_built_graphs(gpu):
    N = 300
    offsets, nbr = np.arange(N + 1, dtype=np.int64), np.arange(N, dtype=np.int32)          # self-edges only
    picks, gain, covered = _greedy_both(offsets, nbr, N + 2)
    assert picks.tolist() == list(range(N)) + [-1, -1] and gain.tolist() == [1] * N + [0, 0] and covered.all()
    A = np.eye(N, dtype=bool)                                              # a star round row 5
    A[5, :] = A[:, 5] = True
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum(A.sum(axis=1))
    nbr = np.nonzero(A)[1].astype(np.int32)
    picks, gain, covered = _greedy_both(offsets, nbr, 3)
    assert picks.tolist() == [5, -1, -1] and gain.tolist() == [N, 0, 0] and covered.all()
    N, u, d = 6000, 4100, 5000                                             # one row of degree > 4096 among empty rows
    offsets = np.zeros(N + 1, np.int64)
    offsets[u + 1:] = d
    nbr = np.arange(d, dtype=np.int32)
    picks, gain, covered = _greedy_both(offsets, nbr, 2)
    assert picks.tolist() == [u, -1] and gain.tolist() == [d, 0] and covered[:d].all() and not covered[d:].any()
    picks, gain, covered = _greedy_both(offsets, nbr, 2, seeds=(u,))       # the seed's ball covered before the first pick
    assert picks.tolist() == [-1, -1] and covered[:d].all()
    offsets, nbr = np.zeros(N + 1, np.int64), np.zeros(0, np.int32)        # a graph without edges
    picks, gain, covered = _greedy_both(offsets, nbr, 2)
    assert picks.tolist() == [-1, -1] and not covered.any()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _same_info(a, b):
    return (a["delta"] == b["delta"] and a["edges"] == b["edges"] and a["covered"] == b["covered"] and a["exhausted"] == b["exhausted"]
            and np.array_equal(a["gain"], b["gain"]))


def test_probcover_device_equals_the_host_on_integer_blobs(gpu):
    from a_link_amd import cluster, probcover
    X, blob, C0 = blobs([30, 20, 12, 4])
    X, C0 = np.abs(X), np.abs(C0)
    L, R, li, ri = _pair_of(X)
    assert np.array_equal(np.abs(L[li] - R[ri]), X)
    forms = (_dev(X), (_dev(L), _dev(R), _dev(li), _dev(ri)))
    for lab in (np.zeros(0, np.int64), np.flatnonzero(blob == 0)[:2]):
        for delta, n in ((8.0, 4), (3.0, 9), (3.0, 64), (2.0, 5)):
            want, winfo = probcover.probcover(X, lab, n, delta=delta)
            for rows in forms:
                got, info = probcover.probcover_device(rows, lab, n, delta=delta)
                assert np.array_equal(got, want) and got.dtype == np.int64, (delta, n, got, want)
                assert _same_info(info, winfo) and len(set(got.tolist()) & set(lab.tolist())) == 0
    want, winfo = probcover.probcover(X, [], 4, delta=8.0)
    assert blob[want].tolist() == [0, 1, 2, 3] and winfo["gain"].tolist() == [30, 20, 12, 4]
    # delta=None: the purity radius of k-means groups (iters = 0: the centres stay integer rows, so both sides assign exactly)
    assign = cluster.kmeans_device(forms[0], 4, iters=0, centres=_dev(C0))["assign"]
    assert np.array_equal(assign.cpu().numpy(), blob)
    X2 = X.copy()
    X2[:, :2] += np.random.RandomState(1).randint(0, 40, (len(X), 2)).astype(np.float32)    # blobs that touch: impure balls exist
    g2 = cluster.kmeans_device(_dev(X2), 4, iters=0, centres=_dev(C0))["assign"]
    for Xc, g, alpha in ((X, assign, 1.0), (X2, g2, 0.95), (X2, g2, 0.8)):
        hg = g.cpu().numpy()
        assert probcover.purity_radius_device(_dev(Xc), g, alpha) == probcover.purity_radius(Xc, hg, alpha)
        t_dev = tuple(t.cpu().numpy() for t in probcover.nearest_other_device(_dev(Xc), g))
        t_host = probcover.nearest_other(Xc, hg)
        assert np.array_equal(_bits(t_dev[0]), _bits(t_host[0].astype(np.float32))) and np.array_equal(t_dev[1], t_host[1])
        for lab in ([], np.flatnonzero(blob == 1)[:3]):
            want, winfo = probcover.probcover(Xc, lab, 6, groups=hg, alpha=alpha, fill="random", random_state=3)
            got, info = probcover.probcover_device(_dev(Xc), lab, 6, groups=g, alpha=alpha, fill="random", random_state=3)
            assert np.array_equal(got, want) and _same_info(info, winfo) and len(got) == 6
    deg = probcover.ball_count_device(forms[0], 8.0).cpu().numpy()
    assert np.array_equal(deg, np.array([30, 20, 12, 4])[blob])


def _committee(D, members=3):
    from a_link_amd import committee, siamese
    return committee.Bagging([siamese.SiameseNetwork((D,), "c%d" % m, 0.1, seed=80 + m) for m in range(members)], [])


def test_bagging_sampler_and_strategy_name(gpu):
    from a_link_amd import existing_al, learners, probcover
    X, blob, C0 = blobs([30, 20, 12, 4], D=64)
    X = np.abs(X)
    L, R, li, ri = (_dev(a) for a in _pair_of(X))
    lab = np.flatnonzero(blob == 1)[:3]
    bag = _committee(64)
    got = bag.probcover_indexed(L, R, li, ri, lab, 5, delta=3.0)
    want = probcover.probcover_device((L, R, li, ri), lab, 5, delta=3.0)
    host = probcover.probcover(X, lab, 5, delta=3.0)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[0], host[0]) and len(got[0]) == 5 and _same_info(got[1], host[1])
    with pytest.raises(ValueError, match="one feature space"):
        bag.probcover_indexed([L] * 3, [R] * 3, li, ri, lab, 5, delta=3.0)
    # the sampler through ActiveLearner: the labelled rows appended behind the pool, the device route equal to the host route
    assert existing_al.get_strategy_object("probcover_sampling") is probcover.probcover_sampling

    class Estimator(object):
        classes_ = np.array([0, 1])

        def fit(self, X, y, **kw):
            return self
    pool = np.delete(X, lab, axis=0)
    # (delta = 8: three picks cover the pool, the rest is the seeded fill; n_clusters: the purity radius of k-means groups)
    for kw in (dict(delta=3.0), dict(delta=8.0, random_state=1), dict(n_clusters=4, iters=0, random_state=2)):
        learner = learners.ActiveLearner(Estimator(), query_strategy=probcover.probcover_sampling, X_training=X[lab], y_training=np.zeros(3))
        idx, inst = learner.query(_dev(pool), n_instances=5, **kw)
        want, _ = learner.query(pool, n_instances=5, **kw)
        assert np.array_equal(idx, want) and len(idx) == 5 and torch.equal(inst, _dev(pool)[torch.from_numpy(idx).cuda()])


def test_python_refusals(gpu):
    from a_link_amd import probcover
    X = _dev(np.random.RandomState(3).randn(50, 8).astype(np.float32))
    g = torch.zeros(50, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="CUDA"):
        probcover.ball_graph_device(X.cpu(), 1.0)
    with pytest.raises(ValueError, match="float32"):
        probcover.ball_graph_device(X.double(), 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e30):
        with pytest.raises(ValueError, match="delta"):
            probcover.ball_graph_device(X, bad)
    with pytest.raises(ValueError, match="empty"):
        probcover.ball_graph_device(X[:0], 1.0)
    with pytest.raises(ValueError, match="D = 8200"):
        probcover.ball_count_device(torch.zeros((2, 8200), device="cuda"), 1.0)
    for bad in (g[:49], g.long(), g.cpu(), [0] * 50):
        with pytest.raises(ValueError, match="groups"):
            probcover.ball_graph_device(X, 1.0, groups=bad)
    with pytest.raises(ValueError, match="groups"):
        probcover.nearest_other_device(X, None)
    with pytest.raises(ValueError, match=r"\+inf"):
        probcover.purity_radius_device(X, g)                               # one group: no ball is ever impure
    offsets, nbr = probcover.ball_graph_device(X, 3.0)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k ="):
            probcover.max_coverage_device(offsets, nbr, bad)
    with pytest.raises(ValueError, match="offsets"):
        probcover.max_coverage_device(offsets.int(), nbr, 1)
    with pytest.raises(ValueError, match="nbr"):
        probcover.max_coverage_device(offsets, nbr.long(), 1)
    with pytest.raises(ValueError, match="labelled"):
        probcover.max_coverage_device(offsets, nbr, 1, seeds=[50])
    with pytest.raises(ValueError, match="covered"):
        probcover.max_coverage_device(offsets, nbr, 1, covered=torch.zeros(50, device="cuda"))
    run = probcover.probcover_device
    with pytest.raises(ValueError, match="empty"):
        run(X[:0], [], 1, delta=1.0)
    with pytest.raises(ValueError, match="only 47 of the 50 rows"):
        run(X, [0, 1, 2], 48, delta=1.0)
    for bad in ([50], [-1], [1, 1], [0.5]):
        with pytest.raises(ValueError, match="labelled"):
            run(X, bad, 1, delta=1.0)
    with pytest.raises(ValueError, match="n_instances"):
        run(X, [], 0, delta=1.0)
    with pytest.raises(ValueError, match="fill"):
        run(X, [], 1, delta=1.0, fill="nearest")


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    N = 8
    x = torch.zeros((N, 4), device="cuda")
    ind = torch.zeros(N, dtype=torch.int32, device="cuda")
    outs = {"deg": torch.full((N,), -7, dtype=torch.int32, device="cuda"), "t": torch.full((N,), -7.0, device="cuda"),
            "j": torch.full((N,), -7, dtype=torch.int32, device="cuda"), "nbr": torch.full((N * N,), -7, dtype=torch.int32, device="cuda"),
            "mis": torch.full((1,), -7, dtype=torch.int32, device="cuda"), "picks": torch.full((3,), -7, dtype=torch.int32, device="cuda"),
            "gain": torch.full((3,), -7, dtype=torch.int32, device="cuda"), "cov": torch.full((N,), 7, dtype=torch.uint8, device="cuda")}
    offsets = torch.arange(N + 1, dtype=torch.int64, device="cuda") * N
    assert lib.alink_ball_scratch_bytes(0, 4) == 0 and lib.alink_ball_scratch_bytes(2 ** 31, 4) == 0
    assert lib.alink_ball_scratch_bytes(N, 0) == 0 and lib.alink_ball_scratch_bytes(N, 8193) == 0
    assert lib.alink_max_coverage_scratch_bytes(0, 1) == 0 and lib.alink_max_coverage_scratch_bytes(N, 0) == 0
    assert lib.alink_max_coverage_scratch_bytes(2 ** 31, 1) == 0
    need = max(lib.alink_ball_scratch_bytes(N, 4), lib.alink_max_coverage_scratch_bytes(N, 3))
    assert need > 0
    scratch = torch.empty(need + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inf, nan = float("inf"), float("nan")

    def count(x_=x, r=None, li=None, ri=None, N_=N, D=4, group=ind, r2=1.0, deg=outs["deg"], t=outs["t"], j=outs["j"], scratch_ptr=sp):
        return lib.alink_ball_count(gpu.ptr(x_), gpu.ptr(r), gpu.ptr(li), gpu.ptr(ri), N_, D, gpu.ptr(group), r2, gpu.ptr(deg), gpu.ptr(t),
                                    gpu.ptr(j), C.c_void_p(scratch_ptr), st)

    def fill(x_=x, r=None, li=None, ri=None, N_=N, D=4, r2=1.0, off=offsets, E=N * N, nbr=outs["nbr"], mis=outs["mis"], scratch_ptr=sp):
        return lib.alink_ball_fill(gpu.ptr(x_), gpu.ptr(r), gpu.ptr(li), gpu.ptr(ri), N_, D, None, r2, gpu.ptr(off), E, gpu.ptr(nbr),
                                   gpu.ptr(mis), C.c_void_p(scratch_ptr), st)

    def greedy(off=offsets, nbr=outs["nbr"], N_=N, seed=None, S=0, k=3, cov=outs["cov"], picks=outs["picks"], gain=outs["gain"],
               scratch_ptr=sp):
        return lib.alink_max_coverage(gpu.ptr(off), gpu.ptr(nbr), N_, gpu.ptr(seed), S, k, gpu.ptr(cov), gpu.ptr(picks), gpu.ptr(gain),
                                      C.c_void_p(scratch_ptr), st)
    pool = [(dict(x_=None), "NULL"), (dict(scratch_ptr=0), "NULL"), (dict(li=ind), "pair form"), (dict(li=ind, r=x), "pair form"),
            (dict(li=ind, ri=ind), "pair form"), (dict(N_=0), "N=0"), (dict(N_=2 ** 31), "N=2147483648"), (dict(D=0), "D=0"),
            (dict(D=8193), "D=8193"), (dict(r2=0.0), "radius2"), (dict(r2=-1.0), "radius2"), (dict(r2=inf), "radius2"),
            (dict(r2=nan), "radius2"), (dict(scratch_ptr=sp + 4), "aligned")]
    for call, cases in ((count, pool + [(dict(deg=None, t=None, j=None), "NULL"), (dict(group=None), "dev_group"),
                                        (dict(group=None, t=None), "dev_group"), (dict(group=None, j=None), "dev_group")]),
                        (fill, pool + [(dict(off=None), "NULL"), (dict(nbr=None), "NULL"), (dict(mis=None), "NULL"), (dict(E=-1), "E=-1")]),
                        (greedy, [(dict(off=None), "NULL"), (dict(nbr=None), "NULL"), (dict(cov=None), "NULL"), (dict(picks=None), "NULL"),
                                  (dict(gain=None), "NULL"), (dict(scratch_ptr=0), "NULL"), (dict(S=2), "NULL"), (dict(N_=0), "N=0"),
                                  (dict(N_=2 ** 31), "N=2147483648"), (dict(k=0), "k=0"), (dict(k=-2), "k=-2"), (dict(S=-1, seed=ind), "S=-1"),
                                  (dict(scratch_ptr=sp + 8), "aligned")])):
        for kw, text in cases:
            assert call(**kw) == -1, (call.__name__, kw)                   # ALINK_EINVAL
            assert text in lib.alink_last_error().decode(), (call.__name__, kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(greedy(k=0), "alink_max_coverage")
    torch.cuda.synchronize()
    assert all(bool((v == (7 if k == "cov" else -7)).all()) for k, v in outs.items())       # a refused call launches nothing
    # each output of the count may be NULL, not all three
    assert count(t=None, j=None, group=None) == 0 and count(deg=None) == 0
    torch.cuda.synchronize()
    assert outs["deg"].cpu().tolist() == [N] * N and bool((outs["t"] == inf).all()) and outs["j"].cpu().tolist() == [-1] * N
    assert fill() == 0 and greedy(seed=ind[:1] + 3, S=1) == 0
    torch.cuda.synchronize()
    assert outs["mis"].item() == 0 and outs["nbr"].cpu().tolist() == list(range(N)) * N
    assert outs["picks"].cpu().tolist() == [-1] * 3 and outs["gain"].cpu().tolist() == [0] * 3      # (covered came in nonzero)
    # offsets that do not fit the balls: nothing is written outside a row's span or [0, E), and the rows are counted
    short = torch.arange(N + 1, dtype=torch.int64, device="cuda") * (N - 1)
    outs["nbr"].fill_(-7)
    assert fill(off=short, E=N * (N - 1)) == 0
    torch.cuda.synchronize()
    assert outs["mis"].item() == N and bool((outs["nbr"][N * (N - 1):] == -7).all())
    assert outs["nbr"][:N * (N - 1)].cpu().tolist() == list(range(N - 1)) * N
