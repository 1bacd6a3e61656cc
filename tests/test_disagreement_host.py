"""CPU: the query-by-committee measures and samplers of a-link_amd/disagreement.py (modAL.disagreement, which the reference
imports at code/learners.py:12).  modAL is not a dependency: the float64 reference restates its formulas with
scipy.stats.entropy."""
import os
import re

import numpy as np
import pytest
from scipy.stats import entropy

import a_link_amd  # noqa: F401
from a_link_amd import _abi, disagreement as D, learners, uncertainty as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN2, LN3 = np.log(2.0), np.log(3.0)
H13 = -(2.0 / 3.0) * np.log(2.0 / 3.0) - (1.0 / 3.0) * np.log(1.0 / 3.0)      # H(2/3, 1/3) = 0.636514...


class _Estimator:
    """a fitted classifier whose probabilities are a fixed function of the LEFT features"""

    def __init__(self, W, classes=(0, 1, 2)):
        self.W = np.asarray(W, np.float64)
        self.classes_ = np.asarray(classes)

    def predict_proba(self, X):
        z = np.asarray(X[0], np.float64) @ self.W
        e = np.exp(z - z.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)

    def predict(self, X):
        return self.classes_[np.argmax(self.predict_proba(X), axis=1)]

    def fit(self, X, y, **kw):
        return self


class _FixedCommittee:
    """duck-typed committee answering from arrays: votes (P, M) and / or member probabilities (P, M, C)"""

    def __init__(self, votes=None, proba=None, classes=(0, 1, 2)):
        self.votes, self.proba, self.classes_ = votes, proba, np.asarray(classes)

    def __len__(self):
        return (self.votes if self.votes is not None else self.proba).shape[1]

    def vote(self, X):
        return self.votes

    def vote_proba(self, X):
        return self.proba

    def predict_proba(self, X):
        return self.proba.mean(axis=1)


def _committee(n_members=4, d=6, n_classes=3, seed=0, query_strategy=None):
    rng = np.random.RandomState(seed)
    ls = [learners.ActiveLearner(_Estimator(rng.randn(d, n_classes) * 2.0, classes=range(n_classes))) for _ in range(n_members)]
    return learners.Committee(ls, **({} if query_strategy is None else {"query_strategy": query_strategy}))


def _pairs(n=40, d=6, seed=1):
    rng = np.random.RandomState(seed)
    return [rng.randn(n, d), rng.randn(n, d)]


def test_vote_entropy_known_answers():
    votes = np.array([[0, 1, 0], [1, 1, 2], [0, 1, 2], [2, 2, 2]], dtype=np.float64)
    X = [np.zeros((4, 1)), np.zeros((4, 1))]
    got = D.vote_entropy(_FixedCommittee(votes=votes), X)
    np.testing.assert_allclose(got, [H13, H13, LN3, 0.0], atol=1e-15)
    np.testing.assert_allclose(got, [0.6365141682948128, 0.6365141682948128, 1.0986122886681098, 0.0], atol=1e-12)


def test_two_opposed_members_known_answers():
    proba = np.array([[[1.0, 0.0], [0.0, 1.0]]])                       # one pair, members [1, 0] and [0, 1]
    c = _FixedCommittee(proba=proba, classes=(0, 1))
    X = [np.zeros((1, 1)), np.zeros((1, 1))]
    np.testing.assert_array_equal(c.predict_proba(X), [[0.5, 0.5]])
    np.testing.assert_allclose(D.consensus_entropy(c, X), [LN2], atol=1e-15)
    np.testing.assert_allclose(D.KL_max_disagreement(c, X), [LN2], atol=1e-15)


def test_identical_members_do_not_disagree():
    row = np.random.RandomState(3).dirichlet(np.ones(5), size=7)        # (7, 5)
    proba = np.repeat(row[:, None, :], 4, axis=1)
    got = D.KL_max_disagreement(_FixedCommittee(proba=proba, classes=range(5)), [np.zeros((7, 1))] * 2)
    np.testing.assert_allclose(got, np.zeros(7), atol=1e-15)


def test_measures_equal_scipy_expressions():
    com, X = _committee(), _pairs()
    P, M, C = 40, len(com), com.n_classes_
    votes, pv = com.vote(X), com.vote_proba(X)
    assert votes.shape == (P, M) and pv.shape == (P, M, C)
    want_ve = np.array([entropy([np.sum(votes[i] == c) / float(M) for c in com.classes_]) for i in range(P)])
    want_ce = np.array([entropy(pv[i].mean(axis=0)) for i in range(P)])
    want_kl = np.array([max(entropy(pv[i, m], pv[i].mean(axis=0)) for m in range(M)) for i in range(P)])
    assert want_ve.max() > 0.5 and want_kl.max() > 0.1                   # members that do disagree
    np.testing.assert_allclose(D.vote_entropy(com, X), want_ve, atol=1e-12, rtol=0)
    np.testing.assert_allclose(D.consensus_entropy(com, X), want_ce, atol=1e-12, rtol=0)
    np.testing.assert_allclose(D.KL_max_disagreement(com, X), want_kl, atol=1e-12, rtol=0)
    # the array forms Bagging's host path uses are the same formulas
    np.testing.assert_allclose(D.votes_entropy(votes, com.classes_), want_ve, atol=1e-12, rtol=0)
    np.testing.assert_allclose(D.proba_consensus_entropy(pv), want_ce, atol=1e-12, rtol=0)
    np.testing.assert_allclose(D.proba_max_disagreement(pv), want_kl, atol=1e-12, rtol=0)


@pytest.mark.parametrize("sampler,measure", [("consensus_entropy_sampling", "consensus_entropy"),
                                             ("max_disagreement_sampling", "KL_max_disagreement")])
def test_samplers_pick_the_largest_measure(sampler, measure):
    com, X = _committee(), _pairs()
    k = 7
    values = getattr(D, measure)(com, X)
    idx, inst = getattr(D, sampler)(com, X, n_instances=k)
    assert np.array_equal(idx, U.multi_argmax(values, n_instances=k))
    assert set(idx.tolist()) == set(np.argsort(-values)[:k].tolist())
    # the pair-input return shape of the samplers in uncertainty.py: the LEFT rows twice
    assert isinstance(inst, list) and len(inst) == 2
    assert np.array_equal(inst[0], X[0][idx]) and np.array_equal(inst[1], X[0][idx])
    # random tie-break: whatever the shuffle, the same SET where the values are distinct
    for seed in (0, 1):
        np.random.seed(seed)
        ridx, rinst = getattr(D, sampler)(com, X, n_instances=k, random_tie_break=True)
        assert sorted(ridx.tolist()) == sorted(idx.tolist())
        assert np.array_equal(rinst[0], X[0][ridx]) and np.array_equal(rinst[1], X[0][ridx])


def test_random_tie_break_chooses_among_the_tied():
    proba = np.array([[[1.0, 0.0], [0.0, 1.0]]] * 6 + [[[1.0, 0.0], [1.0, 0.0]]] * 6)        # six pairs at ln 2, six at 0
    c = _FixedCommittee(proba=proba, classes=(0, 1))
    X = [np.arange(12.0)[:, None], np.zeros((12, 1))]
    seen = set()
    for seed in range(8):
        np.random.seed(seed)
        idx, _ = D.max_disagreement_sampling(c, X, n_instances=3, random_tie_break=True)
        assert len(set(idx.tolist())) == 3 and set(idx.tolist()) <= set(range(6))
        seen |= set(idx.tolist())
    assert len(seen) > 3                                                # not the same three every time


def test_committee_query_with_a_disagreement_strategy():
    X = _pairs()
    for strategy, measure in ((D.max_disagreement_sampling, D.KL_max_disagreement), (D.consensus_entropy_sampling, D.consensus_entropy),
                              (D.vote_entropy_sampling, None)):
        com = _committee(query_strategy=strategy)
        idx, inst = com.query(X, n_instances=5)
        assert len(idx) == 5 and np.array_equal(inst[0], X[0][idx])
        if measure is not None:
            assert np.array_equal(idx, U.multi_argmax(measure(com, X), n_instances=5))
    assert D.vote_entropy_sampling is learners.vote_entropy_sampling     # re-exported, not copied
    # the default strategy's own measure agrees with the one here
    com = _committee()
    ve = D.vote_entropy(com, X)
    idx, _ = learners.vote_entropy_sampling(com, X, n_instances=5)
    assert np.array_equal(idx, U.multi_argmax(ve, n_instances=5))


def test_not_fitted_committee_scores_zero():
    class _Unfitted(_FixedCommittee):
        def vote(self, X):
            raise U.NotFittedError()
        vote_proba = predict_proba = vote
    c, X = _Unfitted(votes=np.zeros((3, 2))), [np.zeros((3, 1))] * 2
    for f in (D.vote_entropy, D.consensus_entropy, D.KL_max_disagreement):
        assert np.array_equal(f(c, X), np.zeros(3))


def test_entry_point_is_declared_exported_and_bound():
    name = "alink_committee_disagreement"
    header = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name][1]) == 10
    assert hasattr(_abi.load(), name)


def test_new_kernel_uses_no_scratch():
    """the per-pair sums and vote counts must stay in registers at every class capacity (select.usage: the compiler's report)"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "select.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    fn, seen = None, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "disagreement_kernel" in fn:
            seen += 1
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
    assert seen >= 5, seen


def test_bagging_host_path_applies_the_formulas():
    """members that are not device heads: Bagging.disagreement works from their predict outputs"""
    from a_link_amd import committee

    class _Model:
        def __init__(self, W):
            self.e = _Estimator(W)

        def predict(self, X):
            return self.e.predict_proba(X)
    rng = np.random.RandomState(5)
    models = [_Model(rng.randn(6, 3) * 2.0) for _ in range(3)]
    X = _pairs()
    bag = committee.Bagging(models, [])
    pv = np.stack([m.predict(X) for m in models], axis=1)
    np.testing.assert_allclose(bag.disagreement(X, kind="max_disagreement"), D.proba_max_disagreement(pv), atol=1e-15)
    np.testing.assert_allclose(bag.disagreement(X, kind="consensus_entropy"), D.proba_consensus_entropy(pv), atol=1e-15)
    np.testing.assert_allclose(bag.disagreement(X), D.votes_entropy(pv.argmax(axis=2), range(3)), atol=1e-15)
    with pytest.raises(ValueError):
        bag.disagreement(X, kind="entropy")
