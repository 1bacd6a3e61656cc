"""CPU: the clustering strategies' host form (a-link_amd/cluster.py: kmeans, kmeans_sampling, diverse_minibatch_sampling) against
sklearn's Lloyd iterations and against the rule's own edge cases; the surface of alink_kmeans; no scratch in its kernels."""
import os
import re

import numpy as np
import pytest

import a_link_amd  # noqa: F401
from a_link_amd import _abi, cluster, existing_al

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1003, 40, 16), (2000, 128, 32), (777, 7, 5), (1500, 512, 24)]


def mixture(N, D, K, seed):
    """a seeded Gaussian mixture of K components whose first K rows come one from each component (the initial centres)"""
    rng = np.random.RandomState(seed)
    means = rng.randn(K, D)
    comp = np.concatenate([np.arange(K), rng.randint(0, K, N - K)])
    X = (means[comp] + rng.randn(N, D)).astype(np.float32)
    return X, X[:K].copy()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_kmeans_equals_sklearn_lloyd(case, weighted):
    from sklearn.cluster import KMeans
    N, D, K = SHAPES[case]
    X, C0 = mixture(N, D, K, 50 + case)
    w = np.random.RandomState(9 + case).uniform(0.5, 2.0, N).astype(np.float32) if weighted else None
    T = 6
    got = cluster.kmeans(X, C0, T, weights=w)
    assert got["counts"].min() > 0, "an empty cluster: sklearn would relocate it, the comparison would say nothing"
    for t in range(1, T + 1):                            # (and no cluster empties on the way: every prefix is compared)
        part = cluster.kmeans(X, C0, t, weights=w)
        assert part["counts"].min() > 0
    km = KMeans(n_clusters=K, init=C0.astype(np.float64), n_init=1, algorithm="lloyd", tol=0, max_iter=T)
    km.fit(X.astype(np.float64), sample_weight=None if w is None else w.astype(np.float64))
    # sklearn stops early once the labels repeat; the rule's later passes repeat the fixed point, so the ends agree
    if km.n_iter_ < T:
        assert got["changed"][km.n_iter_:].sum() == 0 or got["changed"][-1] == 0
    assert np.array_equal(got["assign"], km.labels_)
    assert abs(got["inertia"][-1] - km.inertia_) <= 1e-9 * km.inertia_
    scale = np.abs(km.cluster_centers_).max()
    assert np.abs(got["centres"].astype(np.float64) - km.cluster_centers_).max() <= 2.0 ** -23 * scale
    assert got["assign"].dtype == np.int32 and got["centres"].dtype == np.float32
    assert got["inertia"].shape == (T + 1,) and got["changed"].shape == (T + 1,) and got["changed"][0] == N
    assert (np.diff(got["inertia"]) <= 1e-9 * got["inertia"][0]).all()
    d2 = ((X.astype(np.float64) - got["centres"].astype(np.float64)[got["assign"]]) ** 2).sum(axis=1)
    assert np.array_equal(got["d2"], d2)
    for j in range(K):
        m = np.flatnonzero(got["assign"] == j)
        assert got["nearest"][j] == m[np.argmin(d2[m])] and got["counts"][j] == m.size


def test_ties_go_to_the_lower_centre_and_an_empty_cluster_keeps_its_centre():
    X = np.array([[0., 0.], [1., 0.], [10., 0.], [11., 1.]], np.float32)
    C = np.array([[0., 0.], [0., 0.], [10., 0.], [100., 100.]], np.float32)
    got = cluster.kmeans(X, C, 0)
    assert got["assign"].tolist() == [0, 0, 2, 2]                   # the second of two identical centres stays empty
    assert got["counts"].tolist() == [2, 0, 2, 0] and got["nearest"].tolist() == [0, -1, 2, -1]
    assert got["changed"].tolist() == [4] and got["wsum"].tolist() == [2., 0., 2., 0.] and np.array_equal(got["centres"], C)
    got = cluster.kmeans(X, C, 1)                                    # ... and keeps its value, as the far centre does
    assert np.array_equal(got["centres"], np.array([[.5, 0.], [0., 0.], [10.5, .5], [100., 100.]], np.float32))
    assert got["assign"].tolist() == [1, 0, 2, 2] and got["changed"].tolist() == [4, 1] and got["counts"].tolist() == [1, 1, 2, 0]
    # a row at equal distance from two different centres
    got = cluster.kmeans(np.array([[1., 0.]]), np.array([[2., 0.], [0., 0.]]), 0)
    assert got["assign"].tolist() == [0] and got["d2"].tolist() == [1.0]


def test_a_cluster_without_weight_keeps_its_centre():
    X = np.array([[0.], [2.], [10.], [12.]], np.float32)
    C = np.array([[1.5], [10.5]], np.float32)
    for bad in (0.0, -1.0, np.nan, np.inf):
        got = cluster.kmeans(X, C, 1, weights=[1, 3, bad, bad])
        assert np.array_equal(got["centres"], np.array([[1.5], [10.5]], np.float32))
        assert got["assign"].tolist() == [0, 0, 1, 1] and got["counts"].tolist() == [2, 2] and got["wsum"].tolist() == [4.0, 0.0]
        assert got["inertia"].tolist() == [1 * 2.25 + 3 * .25] * 2
    got = cluster.kmeans(X, C, 1, weights=[1, 3, 1, 0])
    assert np.array_equal(got["centres"], np.array([[1.5], [10.]], np.float32))


def test_nan_rows_and_non_finite_centres_are_left_out():
    X = np.array([[0., 0.], [np.nan, 0.], [4., 0.], [0., 0.]], np.float32)
    C = np.array([[1., 0.], [np.inf, 0.], [5., 0.]], np.float32)
    got = cluster.kmeans(X, C, 1)
    assert got["assign"].tolist() == [0, -1, 2, 0] and np.isnan(got["d2"][1]) and got["d2"][[0, 2, 3]].tolist() == [0., 0., 0.]
    assert np.array_equal(got["centres"], np.array([[0., 0.], [np.inf, 0.], [4., 0.]], np.float32))
    assert got["counts"].tolist() == [2, 0, 1] and got["nearest"].tolist() == [0, -1, 2]
    assert got["inertia"].tolist() == [2.0 + 1.0, 0.0] and got["changed"].tolist() == [3, 0]


def test_changed_ends_in_zeros_once_a_pass_repeats():
    X, C0 = mixture(777, 7, 5, 53)
    got = cluster.kmeans(X, C0, 40)
    first = int(np.flatnonzero(got["changed"] == 0)[0])
    assert 1 < first < 40 and (got["changed"][first:] == 0).all() and (got["changed"][:first] > 0).all()
    assert len(set(got["inertia"][first:].tolist())) == 1           # (pass first - 1 still moved the centres once more)
    again = cluster.kmeans(X, C0, first)
    assert np.array_equal(again["centres"], got["centres"]) and np.array_equal(again["assign"], got["assign"])


class _Clf(object):
    def __init__(self, proba):
        self.proba = proba

    def predict_proba(self, X):
        return self.proba


def duplicate_pool(seed=4):
    rng = np.random.RandomState(seed)
    base = rng.randn(40, 12).astype(np.float32)
    order = rng.permutation(400)
    L = np.repeat(base, 10, axis=0)[order]
    return L, np.zeros_like(L), base


def test_kmeans_sampling_takes_each_of_40_distinct_rows_once():
    L, R, base = duplicate_pool()
    for X in ([L, R], L):
        idx, inst = cluster.kmeans_sampling(None, X, n_instances=40, random_state=3)
        assert idx.shape == (40,) and idx.dtype == np.int64
        assert len({L[i].tobytes() for i in idx}) == 40
    idx, inst = cluster.kmeans_sampling(None, [L, R], n_instances=40, random_state=3)
    assert np.array_equal(inst[0], L[idx]) and np.array_equal(inst[1], L[idx])          # the kept quirk: the LEFT array twice
    again, _ = cluster.kmeans_sampling(None, [L, R], n_instances=40, random_state=3)
    assert np.array_equal(idx, again)
    # more clusters than distinct rows: the seeding is exhausted, the empty clusters are dropped
    idx, _ = cluster.kmeans_sampling(None, [L, R], n_instances=55, random_state=3)
    assert idx.shape == (40,) and len({L[i].tobytes() for i in idx}) == 40
    idx, _ = cluster.kmeans_sampling(None, [L[:7], R[:7]], n_instances=20, random_state=1)
    assert len(idx) <= 7 and len(set(idx.tolist())) == len(idx)


def test_diverse_minibatch_sampling_stays_inside_the_top_beta_k():
    rng = np.random.RandomState(12)
    L, R = rng.randn(600, 9).astype(np.float32), rng.randn(600, 9).astype(np.float32)
    p = rng.uniform(0.5, 1.0, 600)
    clf = _Clf(np.stack([p, 1 - p], axis=1))
    utility = 1 - p
    for k, beta in ((5, 3), (12, 10), (7, 1), (700, 2)):
        idx, inst = cluster.diverse_minibatch_sampling(clf, [L, R], n_instances=k, beta=beta, random_state=2)
        kk = min(k, 600)
        top = set(np.argsort(-utility.astype(np.float32), kind="stable")[:min(600, beta * kk)].tolist())
        assert 0 < len(idx) <= kk and set(idx.tolist()) <= top and len(set(idx.tolist())) == len(idx)
        assert np.array_equal(inst[0], L[idx]) and np.array_equal(inst[1], L[idx])
    idx, _ = cluster.diverse_minibatch_sampling(clf, [L, R], n_instances=7, beta=1, random_state=2)
    assert set(idx.tolist()) == set(np.argsort(-utility.astype(np.float32), kind="stable")[:7].tolist())   # beta = 1: plain top-k


def test_get_strategy_object_knows_the_two_names():
    assert existing_al.get_strategy_object("kmeans_sampling") is cluster.kmeans_sampling
    assert existing_al.get_strategy_object("diverse_minibatch_sampling") is cluster.diverse_minibatch_sampling


def test_every_refusal_of_the_host_forms():
    X = np.zeros((5, 3), np.float32)
    C = np.zeros((2, 3), np.float32)
    for bad in (np.zeros(5), np.zeros((0, 3)), np.zeros((5, 0))):
        with pytest.raises(ValueError, match="rows"):
            cluster.kmeans(bad, C, 1)
    for bad in (np.zeros((2, 4)), np.zeros(3), np.zeros((0, 3))):
        with pytest.raises(ValueError, match="centres"):
            cluster.kmeans(X, bad, 1)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="iters"):
            cluster.kmeans(X, C, bad)
    with pytest.raises(ValueError, match="weights"):
        cluster.kmeans(X, C, 1, weights=np.ones(4))
    for fn in (cluster.kmeans_sampling, cluster.diverse_minibatch_sampling):
        for bad in (0, -3, 2.5):
            with pytest.raises(ValueError, match="n_instances"):
                fn(_Clf(np.full((5, 2), .5)), [X, X], n_instances=bad)
    for bad in (0, 1.5):
        with pytest.raises(ValueError, match="beta"):
            cluster.diverse_minibatch_sampling(_Clf(np.full((5, 2), .5)), [X, X], n_instances=2, beta=bad)
    with pytest.raises(ValueError, match="uncertainty"):
        cluster.diverse_minibatch_sampling(_Clf(np.full((4, 2), .5)), [X, X], n_instances=2)
    for bad in ((0, 1), (cluster.MAX_K + 1, 1), (2, -1), (2.5, 1)):
        with pytest.raises(ValueError):
            cluster._check_k_iters(*bad)


def test_surface_symbols_declared_exported_bound_and_marked_extension():
    header = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    assert re.search(r"\bsize_t\s+alink_kmeans_scratch_bytes\s*\(", header)
    assert re.search(r"\bint\s+alink_kmeans\s*\(", header)
    assert len(_abi.PROTOTYPES["alink_kmeans_scratch_bytes"][1]) == 3 and len(_abi.PROTOTYPES["alink_kmeans"][1]) == 19
    lib = _abi.load()
    assert hasattr(lib, "alink_kmeans") and hasattr(lib, "alink_kmeans_scratch_bytes")
    assert lib.alink_kmeans_scratch_bytes(0, 4, 4) == 0 and lib.alink_kmeans_scratch_bytes(10, 4, 8193) == 0
    # a function of the sizes alone, and enough for the float64 partial sums of every (cluster, slice)
    a = lib.alink_kmeans_scratch_bytes(100000, 128, 1024)
    assert a == lib.alink_kmeans_scratch_bytes(100000, 128, 1024) and a % 256 == 0 and a >= 1024 * 4 * 128 * 8 + 2 * 4 * 100000
    from a_link_amd import committee
    for obj in (cluster, cluster.kmeans, cluster.kmeans_device, cluster.kmeans_sampling_device, cluster.diverse_minibatch_device,
                cluster.kmeans_sampling, cluster.diverse_minibatch_sampling):
        assert "EXTENSION" in obj.__doc__, obj
    assert "X11" in cluster.__doc__
    assert "Extension" in committee.Bagging.kmeans_sampling_indexed.__doc__
    assert "Extension" in committee.Bagging.diverse_minibatch_indexed.__doc__


def test_no_kmeans_kernel_spills_to_scratch():
    """the build keeps hipcc's per-kernel resource report beside every object: no kernel of kmeans.hip may use scratch — least
    of all the assignment, whose 64 accumulator registers and running minimum must stay registers across the centre tiles"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "kmeans.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    seen, assign, fn = 0, 0, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            seen += 1
            assign += "km_assign_kernel" in fn
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
    assert assign == 8 and seen >= 8 + 8 + 4 + 2 + 2, (assign, seen)        # assign and dist in eight forms, accum in four, norm in two
