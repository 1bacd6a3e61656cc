"""CPU: the rectangular k-nearest-neighbour rule, the CAL score and the selection of a-link_amd/cal.py on the host — against a
literal double loop with a stable sort, against scipy.stats.entropy, and the zero conventions by hand; the sampler through an
ActiveLearner with a stub estimator; and the compiler's resource report of knn_rect.hip (no kernel may use scratch: the running
lists must live in registers)."""
import os
import re

import numpy as np
import pytest
from scipy.stats import entropy

import a_link_amd  # noqa: F401
from a_link_amd import _abi, cal, existing_al, learners

from test_typiclust_host import int_rows, same_lists

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def double_loop(Q, Cm, k):
    """per query the (d2, index) pairs of the references that count, stably sorted by score -> (idx, d2, found).  A row counts when
    its squared norm is finite in float32."""
    Q, Cm = np.asarray(Q, np.float64), np.asarray(Cm, np.float64)
    N, M = len(Q), len(Cm)
    idx, d2, found = np.full((N, k), -1, np.int32), np.full((N, k), np.nan), np.zeros(N, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        q_ok = np.isfinite((Q * Q).sum(axis=1).astype(np.float32))
        c_ok = np.isfinite((Cm * Cm).sum(axis=1).astype(np.float32))
    for n in range(N):
        cand = []
        for j in range(M):
            if q_ok[n] and c_ok[j]:
                cand.append((float((Cm[j] * Cm[j]).sum() - 2.0 * (Q[n] * Cm[j]).sum()), j))
        cand.sort(key=lambda t: t[0])                                      # stable: ties keep the lower index in front
        cand = cand[:k]
        found[n] = len(cand)
        for p, (_, j) in enumerate(cand):
            idx[n, p], d2[n, p] = j, float(((Q[n] - Cm[j]) ** 2).sum())
    return idx, d2, found


def softmax(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


# ---- 1. the neighbour rule -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,D,k", [(40, 60, 3, 7), (25, 90, 2, 20), (33, 5, 6, 9), (12, 1, 4, 3), (1, 33, 1, 32), (50, 50, 5, 5)])
def test_knn_rect_equals_the_double_loop_on_integer_rows_with_ties(N, M, D, k):
    Q, Cm = int_rows(N, D, lo=-2, hi=2), int_rows(M, D, seed=5, lo=-2, hi=2)
    got, want = cal.knn_rect(Q, Cm, k), double_loop(Q, Cm, k)
    assert same_lists(got, want) is None, same_lists(got, want)
    assert (got[2] == min(k, M)).all() and (got[0][:, min(k, M):] == -1).all() and np.isnan(got[1][:, min(k, M):]).all()
    if M > 2 * k:
        d2 = want[1]
        ties = int((d2[:, 1:] == d2[:, :-1]).sum())
        assert ties > N // 2, ties                                         # the case is about ties


def test_knn_rect_is_not_self_excluding_and_tie_free_rows_match_sklearn():
    from sklearn.neighbors import NearestNeighbors
    rng = np.random.RandomState(3)
    Q, Cm = rng.randn(80, 16), rng.randn(120, 16)
    idx, d2, found = cal.knn_rect(Q, Cm, 10)
    dist, ind = NearestNeighbors(n_neighbors=10, algorithm="brute").fit(Cm).kneighbors(Q)
    assert np.array_equal(idx, ind) and (found == 10).all() and np.allclose(np.sqrt(d2), dist, rtol=1e-9, atol=1e-12)
    own, d0, _ = cal.knn_rect(Cm, Cm, 1)                                   # a set against itself: every row finds itself
    assert np.array_equal(own[:, 0], np.arange(120)) and (d0 == 0).all()


def test_knn_rect_non_finite_rows_on_either_side():
    Q = np.array([[0., 0.], [np.nan, 0.], [3., 0.], [np.inf, 1.], [1e30, 0.]], np.float32)
    Cm = np.array([[1., 0.], [0., np.nan], [4., 0.], [-np.inf, 0.], [0., 0.], [0., 1e30]], np.float32)
    idx, d2, found = cal.knn_rect(Q, Cm, 4)
    assert found.tolist() == [3, 0, 3, 0, 0]                               # NaN, +inf and a norm beyond float32: dead rows
    assert idx.tolist() == [[4, 0, 2, -1], [-1] * 4, [2, 0, 4, -1], [-1] * 4, [-1] * 4]
    assert d2[0, :3].tolist() == [0.0, 1.0, 16.0] and d2[2, :3].tolist() == [1.0, 4.0, 9.0]
    assert np.isnan(d2[[1, 3, 4]]).all() and np.isnan(d2[[0, 2], 3]).all()
    assert same_lists((idx, d2, found), double_loop(Q, Cm, 4)) is None
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k ="):
            cal.knn_rect(Q, Cm, bad)
    with pytest.raises(ValueError, match="D = 2, references D = 3"):
        cal.knn_rect(Q, np.zeros((2, 3)), 1)
    with pytest.raises(ValueError, match="references"):
        cal.knn_rect(Q, np.zeros((0, 2)), 1)


# ---- 2. the score rule -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 7])
def test_cal_scores_equal_scipys_entropy_averaged_over_the_neighbours(C):
    rng = np.random.RandomState(C)
    N, M, k = 60, 25, 6
    p, q = softmax(rng.randn(N, C) * 2).astype(np.float32), softmax(rng.randn(M, C) * 2).astype(np.float32)
    idx = np.stack([rng.permutation(M)[:k] for _ in range(N)]).astype(np.int32)
    idx[::5, 4:] = -1                                                      # lists with found < k
    got = cal.cal_scores(p, q, idx)
    assert got.dtype == np.float32 and got.shape == (N,)
    for n in range(N):
        js = idx[n][idx[n] >= 0]
        want = np.mean([entropy(q[j].astype(np.float64), p[n].astype(np.float64)) for j in js])
        # (scipy normalises both vectors, float32 softmaxes sum to 1 within a few 2^-24: a first-order change of the divergence)
        assert abs(got[n] - want) <= 1e-5 * max(1.0, want), (n, got[n], want)
    assert (got >= -1e-6).all() and got.max() > 0.1


def test_cal_scores_zero_conventions_by_hand():
    p = np.array([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75], [0.0, 1.0]], np.float32)
    q = np.array([[1.0, 0.0], [0.5, 0.5], [0.0, 1.0]], np.float32)
    idx = np.array([[0, 2], [0, -1], [-1, -1], [1, 0]], np.int32)
    got = cal.cal_scores(p, q, idx)
    ln2, floor = np.log(2.0), np.log(2.0 ** -126)
    want = [(ln2 + ln2) / 2,                       # q = 0 terms vanish: each neighbour gives 1 * (log 1 - log 0.5)
            0.0,                                   # q = (1, 0) against p = (1, 0): the zero of p meets the zero of q, nothing is floored in
            0.0,                                   # found = 0
            ((0.5 * (np.log(0.5) - floor) + 0.5 * np.log(0.5)) + (0.0 - floor)) / 2]   # p = 0 floored at 2^-126: finite, and large
    want = np.asarray(want, np.float64)
    assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want)).all() and got[1] == 0 and got[2] == 0, (got, want)
    assert np.isfinite(got).all() and got[3] > 60
    # float64 probabilities are taken as they are; a zero of float64 is floored at the same 2^-126
    assert cal.cal_scores(p.astype(np.float64), q.astype(np.float64), idx).tolist() == got.tolist()
    with pytest.raises(ValueError, match="outside the 3 labelled rows"):
        cal.cal_scores(p, q, np.array([[3], [0], [0], [0]], np.int32))
    with pytest.raises(ValueError, match="C = 3"):
        cal.cal_scores(p, np.ones((2, 3)) / 3, idx)
    with pytest.raises(ValueError, match="idx"):
        cal.cal_scores(p, q, idx[:3])


# ---- 3. the selection ------------------------------------------------------------------------------------------------------
def test_cal_returns_the_top_scores_with_ties_to_the_lower_index():
    # labelled rows at 0 and at 10 on a line, scored (1, 0) and (0, 1); pool rows next to either
    lab = np.array([[0.0], [10.0]])
    p_lab = np.array([[1.0, 0.0], [0.0, 1.0]], np.float32)
    rows = np.array([[1.0], [9.0], [2.0], [8.0], [-1.0], [11.0]])
    p_pool = np.array([[0.5, 0.5], [0.5, 0.5], [0.9, 0.1], [0.5, 0.5], [0.1, 0.9], [0.2, 0.8]], np.float32)
    picks, scores = cal.cal(rows, lab, p_pool, p_lab, 6, k_nn=1)
    idx = cal.knn_rect(rows, lab, 1)[0]
    assert idx[:, 0].tolist() == [0, 1, 0, 1, 0, 1]
    assert np.array_equal(scores, cal.cal_scores(p_pool, p_lab, idx))
    # row 4 sits at the genuine-looking labelled row but is scored unlike it: the largest score; rows 0, 1, 3 tie at log 2
    assert scores[0] == scores[1] == scores[3] == np.float32(np.log(2.0))
    assert picks.tolist() == [4, 0, 1, 3, 5, 2] and picks.dtype == np.int64
    assert cal.cal(rows, lab, p_pool, p_lab, 2, k_nn=1)[0].tolist() == [4, 0]
    assert cal.cal(rows, lab, p_pool, p_lab, 50, k_nn=1)[0].tolist() == [4, 0, 1, 3, 5, 2]       # clipped to the pool
    assert cal.cal(rows, lab, p_pool, p_lab, 3, k_nn=1, exclude=[0, 4])[0].tolist() == [1, 3, 5]
    both, s2 = cal.cal(rows, lab, p_pool, p_lab, 1, k_nn=5)                # k beyond the labelled set: the mean over both
    assert np.array_equal(s2, cal.cal_scores(p_pool, p_lab, np.array([[0, 1, -1, -1, -1], [1, 0, -1, -1, -1]] * 3, np.int32)))
    with pytest.raises(ValueError, match="n_instances"):
        cal.cal(rows, lab, p_pool, p_lab, 0)
    with pytest.raises(ValueError, match="excluded"):
        cal.cal(rows, lab, p_pool, p_lab, 1, exclude=list(range(6)))


class _Estimator:
    """a fitted two-class stub over array or pair input: probabilities from a fixed projection of the row / of |left - right|"""

    def __init__(self, w):
        self.w = np.asarray(w, np.float64)
        self.classes_ = np.array([0, 1])

    def predict_proba(self, X):
        rows = np.abs(X[0] - X[1]) if isinstance(X, list) else X
        p = 1.0 / (1.0 + np.exp(-(rows @ self.w)))
        return np.stack([p, 1.0 - p], axis=1)

    def fit(self, X, y, **kw):
        return self


def test_cal_sampling_through_an_active_learner():
    assert existing_al.get_strategy_object("cal_sampling") is cal.cal_sampling
    rng = np.random.RandomState(8)
    D = 6
    pool, train = rng.randn(90, D), rng.randn(12, D)
    est = _Estimator(rng.randn(D))
    learner = learners.ActiveLearner(est, query_strategy=cal.cal_sampling, X_training=train, y_training=np.zeros(12))
    idx, inst = learner.query(pool, n_instances=7, k_nn=4)
    want, scores = cal.cal(pool, train, est.predict_proba(pool), est.predict_proba(train), 7, k_nn=4)
    assert np.array_equal(idx, want) and np.array_equal(inst, pool[want]) and len(set(idx.tolist())) == 7
    assert np.array_equal(np.sort(scores)[::-1][:7], scores[idx])
    # pair input: the rows are |left - right| on both sides, and the kept quirk of the return value
    left, tl = rng.randn(90, D), rng.randn(12, D)
    right, tr = left - pool, tl - train
    learner = learners.ActiveLearner(est, query_strategy=cal.cal_sampling, X_training=[tl, tr], y_training=np.zeros(12))
    idx2, inst2 = learner.query([left, right], n_instances=7, k_nn=4)
    want2, _ = cal.cal(np.abs(left - right), np.abs(tl - tr), est.predict_proba([left, right]), est.predict_proba([tl, tr]), 7, k_nn=4)
    assert np.array_equal(idx2, want2) and isinstance(inst2, list) and np.array_equal(inst2[0], left[want2]) and np.array_equal(inst2[1], left[want2])
    # nothing labelled yet: there is nothing to contrast with
    with pytest.raises(ValueError, match="at least one labelled row"):
        learners.ActiveLearner(est, query_strategy=cal.cal_sampling).query(pool, n_instances=3)


# ---- 4. the build's resource report ----------------------------------------------------------------------------------------
def test_no_knn_rect_kernel_spills_to_scratch_and_the_list_kernels_keep_two_waves():
    """kr_list_kernel's running lists are register arrays that only constant indices reach (knn.hip's test says why that
    matters); it keeps kn_list_kernel's two waves per SIMD in every form but KK = 32 on row tables read with scalar loads.  The
    build keeps the compiler's per-kernel report beside the object (a-link_amd/lib/obj/knn_rect.usage)."""
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("the library has not been built: run __graft_entry__.build() first")
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "knn_rect.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    fn, seen, lists = None, 0, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            seen += 1
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
        m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", ln)
        if m and fn and "kr_list_kernel" in fn:
            lists += 1
            assert int(m.group(1)) >= (1 if "ILi32ELb0ELb0E" in fn else 2), "%s: %s waves per SIMD" % (fn, m.group(1))
    assert seen >= 21 and lists == 12, (seen, lists)
