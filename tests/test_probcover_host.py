"""CPU: the delta-ball graph, the purity radius and the greedy maximum coverage of a-link_amd/probcover.py on the host — against a
literal double loop, sklearn's radius_neighbors_graph and an edge-deletion restatement of the paper's greedy; the float32
acceptance predicate the GPU test applies to alink_ball_count / alink_ball_fill, shown to pass a float32 stand-in of the rule and
to fail every mutant of it; and the compiler's resource report of probcover.hip (no kernel may use scratch)."""
import os
import re

import numpy as np
import pytest

from a_link_amd import probcover
from test_typiclust_host import blobs, int_rows, random_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the real-valued inputs of the float32 predicate, here and on the GPU: RandomState(N + D).randn(N, D) as float32
REAL_SHAPES = [(300, 33), (257, 130), (300, 3), (129, 512)]
QUANTILES = (0.02, 0.10, 0.50)
BAND_SHARE = 2e-3                                          # the share of pairs the predicate may be unable to judge


def real_rows(N, D):
    return np.random.RandomState(N + D).randn(N, D).astype(np.float32)


def pair_d2(X):
    """float64 squared distances by direct differences"""
    X = np.asarray(X, np.float64)
    return ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)


def quantile_radius2(X, q):
    """the float32 nearest to the q-quantile of the off-diagonal squared distances"""
    d2 = pair_d2(X)
    return np.float32(np.quantile(d2[~np.eye(len(X), dtype=bool)], q))


def delta_of(radius2):
    """a delta whose probcover.radius2_of is the float32 `radius2` exactly"""
    delta = float(np.sqrt(np.float64(np.float32(radius2))))
    assert probcover.radius2_of(delta) == np.float32(radius2)
    return delta


def dense(offsets, nbr, N=None):
    """CSR -> boolean (N, N)"""
    offsets = np.asarray(offsets, np.int64)
    N = len(offsets) - 1 if N is None else N
    A = np.zeros((N, N), bool)
    A[np.repeat(np.arange(N), np.diff(offsets)), np.asarray(nbr, np.int64)] = True
    return A


def csr(A):
    offsets = np.zeros(len(A) + 1, np.int64)
    offsets[1:] = np.cumsum(A.sum(axis=1))
    return offsets, np.nonzero(A)[1].astype(np.int32)


def loop_graph(X, radius2, groups=None):
    """the literal double loop over the rule -> list of neighbour lists"""
    X = np.asarray(X, np.float64)
    N = len(X)
    g = np.zeros(N, np.int64) if groups is None else np.asarray(groups)
    with np.errstate(invalid="ignore", over="ignore"):
        ok = [g[n] >= 0 and bool(np.isfinite(np.float32((X[n] * X[n]).sum()))) for n in range(N)]
    out = []
    for n in range(N):
        out.append([j for j in range(N) if ok[n] and ok[j] and (j == n or float(((X[n] - X[j]) ** 2).sum()) < float(radius2))])
    return out


def graph_within_float32_bound(X, radius2, offsets, nbr, groups=None):
    """The acceptance predicate of a float32 ball graph.  Structure first: offsets ascend from 0 to len(nbr), every row's
    neighbours are strictly ascending indices inside the pool.  Then, against the float64 graph of the same float32 radius2
    (diagonal included, rows that are not eligible empty): every pair on which the two differ must have
    |d2_64 - radius2| <= g (|x_n|^2 + |x_j|^2 + 2 |x_n| |x_j|), g = (D + 8) 2^-24 — the bound of a D-term float32 chain and the
    constant of test_typiclust_host.within_float32_bound.
    -> (failures: list of str, pairs that differ, share of off-diagonal pairs inside the band — those the predicate cannot judge)"""
    X = np.asarray(X, np.float64)
    N, D = X.shape
    offsets, nbr = np.asarray(offsets, np.int64), np.asarray(nbr, np.int64)
    fails = []
    if offsets.shape != (N + 1,) or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != len(nbr):
        return ["offsets are not an exclusive prefix sum ending at len(nbr)"], -1, 0.0
    if len(nbr) and (nbr.min() < 0 or nbr.max() >= N):
        return ["a neighbour outside the pool"], -1, 0.0
    inner = np.ones(len(nbr), bool)
    inner[offsets[:-1][np.diff(offsets) > 0]] = False                      # (the first entry of a row has no predecessor)
    if (np.diff(nbr)[inner[1:]] <= 0).any():
        fails.append("a row's neighbours are not strictly ascending")
    gr = np.zeros(N, np.int64) if groups is None else np.asarray(groups, np.int64)
    sq = (X * X).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        alive = (gr >= 0) & np.isfinite(sq.astype(np.float32))
    Xa, sqa = np.where(alive[:, None], X, 0.0), np.where(alive, sq, 0.0)
    d2 = pair_d2(Xa)
    norm = np.sqrt(sqa)
    band = (D + 8) * 2.0 ** -24 * (sqa[:, None] + sqa[None, :] + 2.0 * norm[:, None] * norm[None, :])
    want = ((d2 < np.float64(radius2)) | np.eye(N, dtype=bool)) & alive[:, None] & alive[None, :]
    got = dense(offsets, nbr, N)
    differ = got != want
    close = np.abs(d2 - np.float64(radius2)) <= band
    bad = differ & ~(close & alive[:, None] & alive[None, :])
    for n, j in zip(*np.nonzero(bad)):
        if len(fails) < 8:
            fails.append("pair (%d, %d): d2 = %.9g against radius2 = %.9g, band %.3g, %s" % (n, j, d2[n, j], radius2, band[n, j],
                                                                                         "reported" if got[n, j] else "left out"))
    off = ~np.eye(N, dtype=bool) & alive[:, None] & alive[None, :]
    return fails, int(differ.sum()), float(close[off].mean()) if off.any() else 0.0


def standin_graph(X, radius2, mutant=None):
    """a NumPy float32 stand-in of the device rule — a GEMM-form dot in BLAS's summation order, not the kernel's chain — and, with
    `mutant`, one wrong kernel: 'le' (`<=` for `<`), 'tile' (the last tile of 128 candidates never looked at), 'self' (self left
    out), 'asym' (the score |x_j|^2 - 2 x_n . x_j, the row's own norm forgotten), 'order' (neighbours descending)
    -> (offsets, nbr)"""
    X = np.asarray(X, np.float32)
    N = len(X)
    xn = (X * X).sum(axis=1)
    t = ((xn[None, :] if mutant == "asym" else xn[:, None] + xn[None, :]) - np.float32(2) * (X @ X.T)).astype(np.float32)
    edge = (t <= np.float32(radius2)) if mutant == "le" else (t < np.float32(radius2))
    if mutant == "self":
        edge &= ~np.eye(N, dtype=bool)
    else:
        edge |= np.eye(N, dtype=bool)
    if mutant == "tile":
        edge[:, 128 * ((N - 1) // 128):] = False
    offsets, nbr = csr(edge)
    if mutant == "order":
        nbr = np.concatenate([nbr[offsets[n]:offsets[n + 1]][::-1] for n in range(N)]) if len(nbr) else nbr
    return offsets, nbr


def edge_deletion_greedy(offsets, nbr, k, seeds=()):
    """The paper's description, restated with explicit edge deletion: a directed graph with an edge u -> v for v in ball(u); when
    a vertex is covered every edge INTO it is deleted; the next query is the vertex of largest out-degree (the lowest such)."""
    N = len(offsets) - 1
    out = [set(np.asarray(nbr[offsets[u]:offsets[u + 1]]).tolist()) for u in range(N)]
    balls = [sorted(s) for s in out]
    covered = np.zeros(N, np.uint8)

    def cover(u):
        for v in balls[u]:
            if not covered[v]:
                covered[v] = 1
                for w in range(N):
                    out[w].discard(v)
    for s in seeds:
        cover(s)
    picks, gain = np.full(k, -1, np.int32), np.zeros(k, np.int32)
    for t in range(k):
        degree = [len(s) for s in out]
        u = max(range(N), key=lambda w: (degree[w], -w))
        if degree[u] == 0:
            break
        picks[t], gain[t] = u, degree[u]
        cover(u)
    return picks, gain, covered


def random_csr(N, seed=0, top=6, self_edges=True):
    """a random directed CSR graph whose degrees take few values: heavy ties"""
    rng = np.random.RandomState(3000 + N + seed)
    A = np.zeros((N, N), bool)
    for u in range(N):
        d = min(N, int(rng.randint(0, top + 1)))
        A[u, rng.choice(N, d, replace=False)] = True
        if self_edges and d:
            A[u, u] = True
    return csr(A)


# ---- 1. the graph ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,r2,G", [(60, 3, 9, None), (90, 2, 2, 3), (33, 1, 1, 1), (70, 4, 16, 40), (5, 6, 16, None)])
def test_ball_graph_equals_the_double_loop_on_integer_rows_with_boundary_ties(N, D, r2, G):
    X = int_rows(N, D, lo=-2, hi=2)
    g = None if G is None else random_groups(N, G)
    d2 = pair_d2(X)
    assert (d2 == r2).any() and (d2 < r2).any()                            # pairs exactly on the radius: the comparison is strict
    offsets, nbr = probcover.ball_graph(X, delta_of(r2), g)
    want = loop_graph(X, r2, g)
    assert offsets.dtype == np.int64 and nbr.dtype == np.int32
    assert [nbr[offsets[n]:offsets[n + 1]].tolist() for n in range(N)] == want
    A = dense(offsets, nbr)
    assert np.array_equal(A, A.T)                                          # symmetric
    alive = np.ones(N, bool) if g is None else g >= 0
    assert A[np.arange(N), np.arange(N)][alive].all() and not A[~alive].any() and not A[:, ~alive].any()
    assert not (A & (d2 >= r2) & ~np.eye(N, dtype=bool)).any()


@pytest.mark.parametrize("N,D,q", [(200, 16, 0.05), (150, 64, 0.3), (40, 5, 0.6)])
def test_ball_graph_equals_sklearns_radius_graph_on_tie_free_rows(N, D, q):
    from sklearn.neighbors import radius_neighbors_graph
    X = np.random.RandomState(N).randn(N, D)
    r2 = quantile_radius2(X, q)
    delta = delta_of(r2)
    offsets, nbr = probcover.ball_graph(X, delta)
    want = radius_neighbors_graph(X, delta, mode="connectivity", include_self=True).toarray() > 0
    got = dense(offsets, nbr)
    d2 = pair_d2(X)
    assert np.abs(d2 - np.float64(r2))[~np.eye(N, dtype=bool)].min() > 1e-9     # tie-free: `<` and `<=` agree
    assert np.array_equal(got, want) and np.array_equal(got, got.T) and got.diagonal().all()
    assert N < len(nbr) < N * N


def test_rows_that_are_not_eligible():
    X = np.array([[0., 0.], [np.nan, 0.], [1., 0.], [np.inf, 1.], [0., 1.], [1e30, 0.], [0., 0.]], np.float32)
    offsets, nbr = probcover.ball_graph(X, 1.25)
    lists = [nbr[offsets[n]:offsets[n + 1]].tolist() for n in range(len(X))]
    assert lists == [[0, 2, 4, 6], [], [0, 2, 6], [], [0, 4, 6], [], [0, 2, 4, 6]]    # NaN, +inf, a norm beyond float32: no ball
    g = np.array([0, 0, -1, 0, 1, 0, -3], np.int32)
    offsets, nbr = probcover.ball_graph(X, 1.25, g)
    assert [nbr[offsets[n]:offsets[n + 1]].tolist() for n in range(len(X))] == [[0, 4], [], [], [], [0, 4], [], []]
    t_other, j_other = probcover.nearest_other(X, g)
    assert j_other.tolist() == [4, -1, -1, -1, 0, -1, -1] and t_other[[0, 4]].tolist() == [1.0, 1.0] and np.isinf(t_other[[1, 2, 3, 5, 6]]).all()
    picks, gain, covered = probcover.max_coverage(offsets, nbr, 3)
    assert picks.tolist() == [0, -1, -1] and gain.tolist() == [2, 0, 0] and covered.tolist() == [1, 0, 0, 0, 1, 0, 0]
    for bad in (0.0, -1.0, np.inf, np.nan, 1e30):
        with pytest.raises(ValueError, match="delta"):
            probcover.ball_graph(X, bad)
    with pytest.raises(ValueError, match="groups"):
        probcover.ball_graph(X, 1.0, np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="rows"):
        probcover.ball_graph(np.zeros((0, 3)), 1.0)


# ---- 2. the purity radius ----------------------------------------------------------------------------------------------------
def _impure(t_other, alive, r2):
    return int((t_other[alive] < np.float64(np.float32(r2))).sum())


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("alpha", [0.95, 0.8, 1.0])
def test_purity_radius_is_the_largest_radius_pure_enough(integer, alpha):
    if integer:
        X, blob, _ = blobs([30, 20, 12, 4])
        X[:, :2] += np.random.RandomState(1).randint(-30, 31, (len(X), 2))  # blobs that touch: many distinct t_other
    else:
        rng = np.random.RandomState(5)
        blob = rng.randint(0, 3, 120)
        X = (rng.randn(120, 6) + 2.0 * np.eye(6)[blob]).astype(np.float32)
    g = blob.astype(np.int32)
    g[[3, 17]] = -1
    alive = g >= 0
    M = int(alive.sum())
    m = int(np.floor((1 - alpha) * M))
    t_other, j_other = probcover.nearest_other(X, g)
    d2 = pair_d2(X)
    for n in np.flatnonzero(alive):                                        # the double loop
        others = [(d2[n, j], j) for j in range(len(X)) if alive[j] and g[j] != g[n]]
        assert j_other[n] == min(others)[1] and abs(t_other[n] - min(others)[0]) <= 1e-9 * max(1.0, min(others)[0])
    assert (j_other[~alive] == -1).all() and np.isinf(t_other[~alive]).all()
    delta = probcover.purity_radius(X, g, alpha)
    r2 = probcover.radius2_of(delta)
    assert _impure(t_other, alive, r2) <= m                                # pure enough at the radius ...
    assert _impure(t_other, alive, np.nextafter(r2, np.float32(np.inf))) > m      # ... and not one float32 above it
    # the scan: every distinct t_other, at the value and at the next float above it — none beyond r2 is pure enough
    for v in np.unique(t_other[alive]):
        lo = np.float32(v)
        for cand in (lo, np.nextafter(lo, np.float32(np.inf))):
            assert (_impure(t_other, alive, cand) <= m) == (cand <= r2), (v, cand, r2)
    # what the radius means for the graph: the balls that hold a row of another group are at most m
    offsets, nbr = probcover.ball_graph(X, delta, g)
    impure = sum(bool((g[nbr[offsets[n]:offsets[n + 1]]] != g[n]).any()) for n in np.flatnonzero(alive))
    assert impure <= m
    assert impure == _impure(t_other, alive, r2)


def test_purity_radius_refusals():
    X, blob, _ = blobs([10, 10])
    with pytest.raises(ValueError, match=r"\+inf"):
        probcover.purity_radius(X, np.zeros(20, np.int32))                 # one group: no ball is ever impure
    with pytest.raises(ValueError, match="alpha"):
        probcover.purity_radius(X, blob.astype(np.int32), 1.5)
    with pytest.raises(ValueError, match="groups"):
        probcover.nearest_other(X, None)
    with pytest.raises(ValueError, match="coincide"):
        probcover.purity_radius(np.zeros((4, 2)), np.array([0, 1, 0, 1], np.int32), 1.0)


# ---- 3. the greedy -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 17, 64, 120])
def test_max_coverage_equals_the_edge_deletion_restatement(N):
    for seed, seeds in ((0, ()), (1, tuple(range(0, N, 7))[:3])):
        offsets, nbr = random_csr(N, seed)
        k = N + 2                                                          # past exhaustion
        picks, gain, covered = probcover.max_coverage(offsets, nbr, k, seeds=seeds)
        want = edge_deletion_greedy(offsets, nbr, k, seeds)
        assert np.array_equal(picks, want[0]) and np.array_equal(gain, want[1]) and np.array_equal(covered, want[2])
        assert picks.dtype == np.int32 and gain.dtype == np.int32 and covered.dtype == np.uint8
        real = picks >= 0
        assert (np.diff(gain[real]) <= 0).all()                            # gains never increase
        assert not real[np.argmin(real):].any() if not real.all() else True    # the tail of -1 is a tail
        assert (gain[~real] == 0).all() and (gain[real] > 0).all() and not real.all()
        seeded = np.zeros(N, bool)
        for s in seeds:
            seeded[nbr[offsets[s]:offsets[s + 1]]] = True
        assert int(seeded.sum()) + int(gain.sum()) == int(covered.sum())   # seeds plus gains are the covered rows
        assert len(set(picks[real].tolist())) == int(real.sum())
        # rows covered beforehand count as a seed's ball would
        pre = np.zeros(N, np.uint8)
        pre[seeded] = 1
        again = probcover.max_coverage(offsets, nbr, k, covered=pre)
        assert all(np.array_equal(a, b) for a, b in zip(again, (picks, gain, covered))) and pre.sum() == seeded.sum()


def test_max_coverage_on_a_ball_graph_and_its_refusals():
    X, blob, _ = blobs([30, 20, 12, 4])
    offsets, nbr = probcover.ball_graph(X, 3.0)
    picks, gain, covered = probcover.max_coverage(offsets, nbr, 70)
    want = edge_deletion_greedy(offsets, nbr, 70)
    assert np.array_equal(picks, want[0]) and np.array_equal(gain, want[1]) and covered.all()
    assert (picks[int(gain.astype(bool).sum()):] == -1).all()
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k ="):
            probcover.max_coverage(offsets, nbr, bad)
    with pytest.raises(ValueError, match="offsets"):
        probcover.max_coverage(offsets[:-1], nbr, 1)
    with pytest.raises(ValueError, match="nbr"):
        probcover.max_coverage(offsets, nbr + 1, 1)
    with pytest.raises(ValueError, match="labelled"):
        probcover.max_coverage(offsets, nbr, 1, seeds=[len(X)])
    with pytest.raises(ValueError, match="covered"):
        probcover.max_coverage(offsets, nbr, 1, covered=np.zeros(3, np.uint8))


def test_probcover_selection_on_integer_blobs():
    X, blob, _ = blobs([30, 20, 12, 4])                                    # inside a blob d2 <= 32, between blobs d2 > 7000
    picks, info = probcover.probcover(X, [], 4, delta=8.0)
    assert blob[picks].tolist() == [0, 1, 2, 3] and info["gain"].tolist() == [30, 20, 12, 4]
    assert picks.tolist() == [int(np.flatnonzero(blob == b)[0]) for b in range(4)]         # every row of a blob ties: the lowest
    assert info["exhausted"] is False and info["edges"] == 30 ** 2 + 20 ** 2 + 12 ** 2 + 4 ** 2 and info["covered"] == 1.0
    assert info["delta"] == 8.0 and picks.dtype == np.int64
    assert probcover.probcover(X, [], 2, delta=8.0)[1]["covered"] == 50 / 66.0
    lab = np.flatnonzero(blob == 0)[:1]
    picks, info = probcover.probcover(X, lab, 65, delta=8.0)               # more than a cover needs: fewer picks come back
    assert info["exhausted"] and blob[picks].tolist() == [1, 2, 3] and info["covered"] == 1.0 and info["gain"].tolist() == [20, 12, 4]
    filled, finfo = probcover.probcover(X, lab, 65, delta=8.0, fill="random", random_state=4)
    assert len(filled) == 65 and np.array_equal(filled[:3], picks) and len(set(filled.tolist())) == 65 and lab[0] not in filled
    assert finfo["exhausted"] and finfo["gain"].tolist() == [20, 12, 4]
    again, _ = probcover.probcover(X, lab, 65, delta=8.0, fill="random", random_state=4)
    assert np.array_equal(again, filled)
    # delta from the purity of a grouping: with alpha = 1 the least distance between rows of different blobs
    picks, info = probcover.probcover(X, lab, 3, groups=blob.astype(np.int32), alpha=1.0)
    d2 = pair_d2(X)
    assert info["delta"] == probcover.purity_radius(X, blob.astype(np.int32), 1.0) == float(np.sqrt(d2[blob[:, None] != blob[None, :]].min()))
    assert blob[picks].tolist() == [1, 2, 3]
    with pytest.raises(ValueError, match="only 65 of the 66 rows"):
        probcover.probcover(X, lab, 66, delta=8.0)
    with pytest.raises(ValueError, match="fill"):
        probcover.probcover(X, lab, 2, delta=8.0, fill="nearest")
    with pytest.raises(ValueError, match="n_instances"):
        probcover.probcover(X, lab, 0, delta=8.0)


class _Learner(object):
    def __init__(self, X_training):
        self.X_training = X_training


def test_probcover_sampling_appends_the_labelled_rows_behind_the_pool():
    from a_link_amd import existing_al
    assert existing_al.get_strategy_object("probcover_sampling") is probcover.probcover_sampling
    X, blob, _ = blobs([30, 20, 12])
    train = X[blob == 0][:3] + 0
    idx, inst = probcover.probcover_sampling(_Learner(train), X, n_instances=2, delta=8.0)
    want, _ = probcover.probcover(np.vstack([X, train]), np.arange(len(X), len(X) + 3), 2, delta=8.0, fill="random")
    assert np.array_equal(idx, want) and np.array_equal(inst, X[idx]) and (idx < len(X)).all()
    assert not (blob[idx] == 0).any()                                      # blob 0 is covered by the labelled rows
    R = np.zeros_like(X)
    idx2, inst2 = probcover.probcover_sampling(_Learner([train, np.zeros_like(train)]), [X, R], n_instances=2, delta=8.0)
    want2, _ = probcover.probcover(np.abs(np.vstack([X, train])), np.arange(len(X), len(X) + 3), 2, delta=8.0, fill="random")
    assert np.array_equal(idx2, want2) and np.array_equal(inst2[0], X[idx2]) and np.array_equal(inst2[1], X[idx2])
    idx3, _ = probcover.probcover_sampling(_Learner(None), X, n_instances=5, n_clusters=3, random_state=1)    # the purity radius
    assert len(idx3) == 5 and len(set(idx3.tolist())) == 5
    idx4, _ = probcover.probcover_sampling(_Learner(None), X, n_instances=62, delta=8.0, random_state=1)      # the fill: always n rows
    assert len(idx4) == 62 and len(set(idx4.tolist())) == 62


# ---- 4. the float32 acceptance predicate -------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D", REAL_SHAPES)
def test_the_float32_graph_predicate_passes_a_stand_in_and_fails_every_mutant(N, D):
    X = real_rows(N, D)
    for q in QUANTILES:
        r2 = quantile_radius2(X, q)
        offsets, nbr = standin_graph(X, r2)
        fails, differ, share = graph_within_float32_bound(X, r2, offsets, nbr)
        print("%d x %d, radius2 at %g: the float32 stand-in differs from float64 on %d pairs; %.3g of the pairs lie in the band"
              % (N, D, q, differ, share))
        assert not fails, fails[:3]
        assert share <= BAND_SHARE
        assert N < len(nbr) < N * N
        for mutant in ("tile", "self", "asym", "order"):
            moff, mnbr = standin_graph(X, r2, mutant)
            assert not (np.array_equal(moff, offsets) and np.array_equal(mnbr, nbr)), mutant
            mfails, _, _ = graph_within_float32_bound(X, r2, moff, mnbr)
            assert mfails, (mutant, q)


def test_the_strict_comparison_shows_on_integer_rows_where_the_check_is_equality():
    """`<=` for `<`: only pairs exactly on the radius show it, and those lie inside any band — on integer rows nothing rounds,
    and the check is equality with the host graph"""
    X = int_rows(257, 3, lo=-2, hi=2)
    r2 = 5
    assert (pair_d2(X) == r2).any()
    want = probcover.ball_graph(X, delta_of(r2))
    got = standin_graph(X, r2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    bad = standin_graph(X, r2, "le")
    assert len(bad[1]) > len(want[1]) and not np.array_equal(bad[0], want[0])
    assert not graph_within_float32_bound(X, np.float32(r2), *got)[0]


# ---- 5. the build's resource report ------------------------------------------------------------------------------------------
def test_no_probcover_kernel_spills_to_scratch():
    """pb_tile_kernel keeps four MFMA accumulators and its decisions in registers that only constant indices reach; one index
    computed at run time would move them to scratch memory, silently and at several times the cost.  The build keeps the
    compiler's per-kernel report beside the object (a-link_amd/lib/obj/probcover.usage)."""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "probcover.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    fn, seen, tiles = None, 0, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            seen += 1
            tiles += "pb_tile_kernel" in fn
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
    assert seen == 20 and tiles == 12, (seen, tiles)
