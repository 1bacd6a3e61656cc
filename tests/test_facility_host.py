"""CPU: the facility-location rule of a-link_amd/facility.py on the host — the gain as the drop of the objective and the pick as
its brute-force argmin on integer rows, the monotone gains, the tie and -1 rules, the labelled rows, the candidate stream, the
sampler through an ActiveLearner; the three entry points' declaration; and the compiler's resource report of facility.hip (no
kernel may use scratch)."""
import os
import re

import numpy as np
import pytest

from a_link_amd import _abi, facility
from test_typiclust_host import int_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def direct_d2(X):
    X = np.asarray(X, np.float64)
    return ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)


def objective_after(d2, cur, s):
    return np.minimum(cur.astype(np.float64), d2[:, s]).sum()


# ---- 1. gain = the drop of the objective; the pick = its brute-force argmin ------------------------------------------------
@pytest.mark.parametrize("N,D,k", [(40, 5, 8), (65, 3, 12)])
def test_gain_is_the_drop_of_the_objective_and_the_pick_its_argmin(N, D, k):
    X = int_rows(N, D)
    d2 = direct_d2(X)
    cur0 = np.full(N, facility.default_cap(X), np.float32)
    assert cur0[0] == 4 * (X.astype(np.float64) ** 2).sum(axis=1).max()
    picks, gain, cur = facility.select(X, cur0, k)
    c = cur0.copy()
    for t in range(k):
        L0 = c.astype(np.float64).sum()
        after = np.array([objective_after(d2, c, s) for s in range(N)])
        best = int(np.argmin(after))                               # the first of equal minima: the lower row
        if after[best] < L0:
            assert picks[t] == best and gain[t] == L0 - after[best], (t, picks[t], best)
            c = np.minimum(c.astype(np.float64), d2[:, best]).astype(np.float32)
        else:
            assert picks[t] == -1 and gain[t] == 0
    assert np.array_equal(cur, c)
    # gains() of all candidates at the start is the drop per single addition, exactly
    g0 = facility.gains(X, cur0)
    assert np.array_equal(g0, cur0.astype(np.float64).sum() - np.array([objective_after(d2, cur0, s) for s in range(N)]))
    # cover() with a list is the minimum over its members, and ignores what is out of range
    got = facility.cover(X, cur0, [3, -1, N, 7, 3])
    assert np.array_equal(got, np.minimum(cur0, np.minimum(d2[:, 3], d2[:, 7])).astype(np.float32))
    assert np.array_equal(cur0, np.full(N, cur0[0], np.float32))                      # the argument is not changed


# ---- 2. a candidate's gain never increases; a picked row's gain is 0 --------------------------------------------------------
def test_gains_never_increase_and_a_picked_row_gains_nothing():
    X = int_rows(50, 4, seed=3)
    cur = np.full(50, facility.default_cap(X), np.float32)
    prev = facility.gains(X, cur)
    picked = []
    for t in range(10):
        p, g, cur = facility.select(X, cur, 1)
        assert g[0] == prev.max() and p[0] == int(np.argmax(prev))
        picked.append(int(p[0]))
        now = facility.gains(X, cur)
        assert (now <= prev).all()
        assert (now[picked] == 0).all()
        prev = now
    assert len(set(picked)) == 10


# ---- 3. ties and -1 ------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lower_position_and_a_covered_pool_gives_minus_one():
    X = np.tile(np.array([[1.0, -2.0, 3.0]], np.float32), (9, 1))
    cur = np.full(9, 7.0, np.float32)
    cand = np.array([[5, 2, 8, 2]], np.int32)
    picks, gain, after = facility.select(X, cur, 1, cand)
    assert picks[0] == 5 and gain[0] == 9 * 7.0 and (after == 0).all()             # position 0 wins, not the lower ROW
    picks, gain, after = facility.select(X, cur, 3)
    assert picks.tolist() == [0, -1, -1] and gain.tolist() == [63.0, 0.0, 0.0]
    # a pool that is covered already: -1 at every step, cur bit for bit what it was (a NaN entry included)
    Y = int_rows(20, 3, seed=1)
    done = np.zeros(20, np.float32)
    done[4] = np.nan
    picks, gain, after = facility.select(Y, done, 4, np.random.RandomState(0).randint(0, 20, (4, 6)))
    assert (picks == -1).all() and (gain == 0).all() and after.tobytes() == done.tobytes()
    # a step without a gain does not end the greedy: a later sample may still gain
    cur = np.full(20, 100.0, np.float32)
    cur = facility.cover(Y, cur, [0])
    picks, gain, _ = facility.select(Y, cur, 2, np.array([[0, 0], [0, 5]]))
    assert picks[0] == -1 and gain[0] == 0 and picks[1] == 5 and gain[1] > 0
    # candidates out of range, or of a row that is not finite, gain 0; a NaN row gives nothing and keeps its cur
    Z = int_rows(12, 3, seed=2)
    Z[3, 1] = np.nan
    Z[6, 0] = np.inf
    cur = np.full(12, 50.0, np.float32)
    g = facility.gains(Z, cur, [3, 6, -1, 12, 0])
    ok = np.ones(12, bool)
    ok[[3, 6]] = False
    assert g[:4].tolist() == [0, 0, 0, 0] and g[4] == np.maximum(50.0 - direct_d2(Z[ok])[:, 0], 0).sum()
    after = facility.cover(Z, cur, [0, 3, 6])
    assert after[3] == 50.0 and after[6] == 50.0 and after[0] == 0


# ---- 4. labelled rows, the fill, clipping ----------------------------------------------------------------------------------
def test_labelled_rows_are_never_picked_and_the_fill_completes_the_batch():
    X = int_rows(30, 4, seed=5)
    lab = np.array([2, 11, 29])
    picks, info = facility.facility(X, lab, 9)
    assert len(picks) == 9 and len(set(picks.tolist())) == 9 and not set(picks.tolist()) & set(lab.tolist())
    assert not info["exhausted"] and len(info["gain"]) == 9 and (np.diff(info["gain"]) <= 0).all()
    cur = facility.cover(X, np.full(30, info["cap"], np.float32), lab)
    want, gain, cur = facility.select(X, cur, 9)
    assert np.array_equal(picks, want) and np.array_equal(info["gain"], gain) and info["objective"] == cur.astype(np.float64).sum()
    # the stochastic greedy draws from sample_candidates; labelled rows may be drawn but gain 0
    picks, _ = facility.facility(X, lab, 9, eps=0.3, random_state=4)
    cand = facility.sample_candidates(30, 9, 0.3, 4)
    want, _, _ = facility.select(X, facility.cover(X, np.full(30, info["cap"], np.float32), lab), 9, cand)
    assert np.array_equal(picks, want[want >= 0]) and not set(picks.tolist()) & set(lab.tolist())
    # duplicates: four distinct rows only — the greedy stops gaining, the fill brings the batch to n
    Y = np.repeat(int_rows(4, 3, seed=7), 5, axis=0)
    picks, info = facility.facility(Y, [0], 8)
    assert len(picks) == 3 and info["exhausted"]
    picks, info = facility.facility(Y, [0], 8, fill="random", random_state=1)
    assert len(picks) == 8 and len(set(picks.tolist())) == 8 and 0 not in picks and info["exhausted"]
    # n_instances beyond the pool is clipped to the rows that are not labelled
    picks, _ = facility.facility(X, lab, 100, fill="random", random_state=0)
    assert sorted(picks.tolist()) == sorted(set(range(30)) - set(lab.tolist()))
    with pytest.raises(ValueError, match="fill"):
        facility.facility(X, lab, 3, fill="nearest")
    with pytest.raises(ValueError, match="n_instances"):
        facility.facility(X, lab, 0)


# ---- 5. the candidate stream ----------------------------------------------------------------------------------------------------
def test_sample_candidates_is_the_stated_stream():
    for N, k, eps, seed in ((1000, 16, 0.01, 3), (50, 7, 0.2, 0), (10, 1, 0.01, 9)):
        R = min(N, int(np.ceil(N / k * np.log(1 / eps))))
        got = facility.sample_candidates(N, k, eps, seed)
        assert got.dtype == np.int32 and got.shape == (k, R) and facility.n_candidates(N, k, eps) == R
        assert np.array_equal(got, np.random.RandomState(seed).randint(0, N, (k, R)))
    assert facility.sample_candidates(1000, 16).shape == (16, min(1000, int(np.ceil(1000 / 16 * np.log(100)))))
    with pytest.raises(ValueError, match="eps"):
        facility.sample_candidates(10, 2, eps=1.0)


# ---- 6. the sampler ------------------------------------------------------------------------------------------------------------
class _Estimator(object):
    def __init__(self, w):
        self.w = np.asarray(w, np.float64)

    def predict_proba(self, X, **kw):
        rows = np.abs(np.asarray(X[0], np.float64) - np.asarray(X[1], np.float64)) if isinstance(X, (list, tuple)) else np.asarray(X, np.float64)
        p = 1.0 / (1.0 + np.exp(-(rows @ self.w)))
        return np.stack([1 - p, p], axis=1)


def test_sampler_through_the_learner_and_the_strategy_name():
    from a_link_amd import existing_al
    from a_link_amd.learners import ActiveLearner
    from a_link_amd.uncertainty import classifier_uncertainty
    assert existing_al.get_strategy_object("facility_sampling") is facility.facility_sampling
    assert "facility_sampling" in existing_al.get_strategy_object.__doc__
    rng = np.random.RandomState(6)
    X = rng.randn(80, 5)
    est = _Estimator(rng.randn(5))
    u = np.asarray(classifier_uncertainty(est, X), np.float32)
    order = np.argsort(-u, kind="stable")
    learner = ActiveLearner(estimator=est, query_strategy=facility.facility_sampling)
    idx, inst = learner.query(X, n_instances=6, beta=3)
    want, _ = facility.facility(X[order[:18]], None, 6, fill="random")
    assert np.array_equal(idx, order[:18][want]) and np.array_equal(inst, X[idx]) and len(set(idx.tolist())) == 6
    # beta = 1: the batch is the top-k uncertain rows in facility order
    idx, _ = learner.query(X, n_instances=6, beta=1)
    assert sorted(idx.tolist()) == sorted(order[:6].tolist())
    # beta = None and beta k >= N: the whole pool (and beta=None never asks the classifier)
    whole, _ = facility.facility(X, None, 6, fill="random")
    assert np.array_equal(facility.facility_sampling(None, X, n_instances=6, beta=None)[0], whole)
    assert np.array_equal(learner.query(X, n_instances=6, beta=20)[0], whole)
    # the stochastic greedy, and pair input with the kept quirk of the returned instances
    left = rng.randn(80, 5)
    right = left - X
    idx, inst = learner.query([left, right], n_instances=5, beta=4, eps=0.2, random_state=2)
    u2 = np.asarray(classifier_uncertainty(est, [left, right]), np.float32)
    top = np.argsort(-u2, kind="stable")[:20]
    want, _ = facility.facility(np.abs(left - right)[top], None, 5, eps=0.2, fill="random", random_state=2)
    assert np.array_equal(idx, top[want]) and isinstance(inst, list) and np.array_equal(inst[0], left[idx]) and np.array_equal(inst[1], left[idx])
    assert len(learner.query(X, n_instances=500)[0]) == 80
    with pytest.raises(ValueError, match="beta"):
        learner.query(X, n_instances=3, beta=0)


# ---- 7. the entry points ---------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alink_hip.h")).read(), flags=re.S)
    for name, kind, nargs in (("alink_facility_gains", "int", 12), ("alink_facility_cover", "int", 11),
                              ("alink_facility_select", "int", 14), ("alink_facility_scratch_bytes", "size_t", 4)):
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), header), name
        assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name][1]) == nargs, name
        assert hasattr(_abi.load(), name)
    lib = _abi.load()
    assert lib.alink_facility_scratch_bytes(0, 8, 1, 1) == 0 and lib.alink_facility_scratch_bytes(10, 8, 11, 1) == 0
    assert lib.alink_facility_scratch_bytes(10, 8, 10, 0) == 0 and lib.alink_facility_scratch_bytes(10, 8193, 10, 1) == 0
    assert lib.alink_facility_scratch_bytes(300, 7, 5, 2) % 256 == 0 and lib.alink_facility_scratch_bytes(300, 7, 5, 2) >= 300 * 4 + 3 * 128 * 8


# ---- 8. the build's resource report -------------------------------------------------------------------------------------------
def test_no_facility_kernel_spills_to_scratch():
    """the float64 accumulators of fl_gains_kernel and the running minimum of fl_cover_kernel must stay in registers beside the
    four MFMA accumulators (facility.usage: the compiler's report)"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "facility.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    fn, seen = None, {}
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
            for key in ("fl_gains_kernel", "fl_cover_kernel", "fl_pick_kernel", "fl_sum_kernel", "pt_norm_kernel"):
                if key in fn:
                    seen[key] = seen.get(key, 0) + 1
    assert seen == {"fl_gains_kernel": 4, "fl_cover_kernel": 4, "fl_pick_kernel": 1, "fl_sum_kernel": 1, "pt_norm_kernel": 4}, seen
