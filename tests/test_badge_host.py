"""CPU: k-means++ seeding on the host (a-link_amd/badge.py) — the draw enumerated exactly on a pool whose weights sum to 64,
exhaustion, the rounded-up product, pick 0, NaN rows, the sampler, the driver's strategy names, the new symbols' surface, and
the kmeanspp kernels' scratch use."""
import os
import re

import numpy as np
import pytest

import a_link_amd  # noqa: F401
from a_link_amd import _abi, badge, egl, existing_al

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENUM_X = np.array([0, 1, 2, 1, 0, 3, 4, 2, 1, 3, 4, 1, 1, 1], np.float64)     # D = 1; after pick 0 = row 0 the weights are x^2, sum 64


def test_exact_enumeration_of_the_second_pick():
    """uniforms[1] = j / 64 for j = 0 .. 63: target = j exactly, the pick is the first row whose cumulative weight exceeds j, so
    the 64 picks hit every row exactly as often as its weight"""
    w = ENUM_X ** 2
    assert w.sum() == 64
    C = np.cumsum(w)
    hist = np.zeros(len(w), np.int64)
    for j in range(64):
        idx, pot = badge.kmeans_pp(ENUM_X[:, None], 2, [0.0, j / 64.0], first=0)
        assert idx.dtype == np.int64 and pot.dtype == np.float64 and idx.shape == pot.shape == (2,)
        assert idx[0] == 0 and np.isnan(pot[0]) and pot[1] == 64.0
        hist[idx[1]] += 1
        assert C[idx[1]] > j and (idx[1] == 0 or C[idx[1] - 1] <= j)
        if j in C:                                                          # on a boundary: the NEXT row with a weight
            assert idx[1] == np.flatnonzero(C > j)[0] and C[idx[1]] - w[idx[1]] == j
    assert np.array_equal(hist, w.astype(np.int64))
    assert hist[0] == 0 and hist[4] == 0                                    # rows 0 and 4 are duplicates of the centre


def exhaustion_pool():
    """96 rows drawn from 12 distinct integer rows"""
    rng = np.random.RandomState(5)
    base = rng.randint(-8, 9, (12, 6)).astype(np.float32)
    assert len({tuple(r) for r in base}) == 12
    take = np.concatenate((np.arange(12), rng.randint(0, 12, 84)))
    rng.shuffle(take)
    return base[take], take


def test_exhaustion_after_the_distinct_rows():
    X, take = exhaustion_pool()
    u = np.random.RandomState(6).random_sample(20)
    for first in (None, 17):
        idx, pot = badge.kmeans_pp(X, 20, u, first=first)
        assert (idx[:12] >= 0).all() and len(set(take[idx[:12]].tolist())) == 12
        assert (idx[12:] == -1).all() and (pot[12:] == 0).all()
        assert np.isnan(pot[0]) and (pot[1:12] > 0).all() and (np.diff(pot[1:12]) < 0).all()
    assert idx[0] == 17


def test_the_largest_uniform_takes_the_last_row_with_a_weight():
    # u = 1 - 2^-53, the largest float64 below 1: the target is the last float64 below T, and only the last row with a
    # weight has a cumulative sum beyond it — never a trailing row without one
    u = 1.0 - 2.0 ** -53
    assert u < 1.0 and u == np.nextafter(1.0, 0.0)
    for x, last in (([0, 1, 1, 1, 0], 3), ([0, 3, 4, 0, 7, 0, 0], 4), ([0, 1e-3, 5e8], 2)):
        X = np.array(x, np.float64)[:, None]
        idx, pot = badge.kmeans_pp(X, 2, [0.0, u], first=0)
        assert idx.tolist() == [0, last] and pot[1] == (X ** 2).sum()


def test_pick_zero_is_the_first_row_of_largest_norm_and_nan_rows_never_win():
    X = np.array([[1, 2], [3, 0], [0, 3], [-3, 0], [2, 2]], np.float64)
    idx, _ = badge.kmeans_pp(X, 1, [0.0])
    assert idx.tolist() == [1]
    Xn = np.vstack((X, [[np.nan, 100.0]], [[1e6, np.nan]]))
    u = np.random.RandomState(1).random_sample(7)
    idx, pot = badge.kmeans_pp(Xn, 7, u)
    assert idx[0] == 1
    assert not set(idx.tolist()) & {5, 6}                                   # a NaN row has no norm and no weight
    assert (idx[:5] >= 0).all() and (idx[5:] == -1).all()
    idx, pot = badge.kmeans_pp(np.full((3, 2), np.nan), 3, u[:3])
    assert idx.tolist() == [-1, -1, -1] and np.isnan(pot[0]) and (pot[1:] == 0).all()
    with pytest.raises(ValueError, match="uniforms"):
        badge.kmeans_pp(X, 3, [0.0, 0.5])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        badge.kmeans_pp(X, 3, [0.0, 1.0, 0.5])
    with pytest.raises(ValueError, match="first"):
        badge.kmeans_pp(X, 3, [0.0, 0.1, 0.5], first=5)


class _Net(object):
    def __init__(self, ws):
        self.ws = ws

    def get_weights(self):
        return self.ws


class _Estimator(object):
    def __init__(self, ws):
        self.siamese_net = _Net(ws)


class _Learner(object):
    def __init__(self, ws):
        self.estimator = _Estimator(ws)


def _case(D=64, h1=128, h2=32, od=2, n=70):
    from oracle import siamese_head as O
    rng = np.random.RandomState(77)
    ws = O.init_weights(D, h1, h2, seed=4, out_dim=od)
    return ws, rng.randn(n, D).astype(np.float32), rng.randn(n, D).astype(np.float32)


def test_badge_sampling_shapes_quirk_and_seed():
    ws, L, R = _case()
    emb = egl.gradient_embedding(ws, [L, R])
    for n in (1, 5, 70):
        want, _ = badge.kmeans_pp(emb, n, np.random.RandomState(3).random_sample(n))
        assert (want >= 0).all() and len(set(want.tolist())) == n
        for clf in (_Learner(ws), _Estimator(ws), _Net(ws)):
            idx, inst = badge.badge_sampling(clf, [L, R], n_instances=n, random_state=3)
            assert idx.shape == (n,) and np.array_equal(idx, want)
            assert np.array_equal(inst[0], L[want]) and np.array_equal(inst[1], L[want])   # the kept quirk: the LEFT array twice
    assert want[0] == np.argmax((emb * emb).sum(axis=1))
    a, _ = badge.badge_sampling(_Net(ws), [L, R], n_instances=12, random_state=9)
    b, _ = badge.badge_sampling(_Net(ws), [L, R], n_instances=12, random_state=9)
    c, _ = badge.badge_sampling(_Net(ws), [L, R], n_instances=12, random_state=10)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    with pytest.raises(TypeError):
        badge.badge_sampling(object(), [L, R])


def test_get_strategy_object_knows_the_new_samplers():
    from a_link_amd import uncertainty
    assert existing_al.get_strategy_object("egl_sampling") is egl.egl_sampling
    assert existing_al.get_strategy_object("badge_sampling") is badge.badge_sampling
    assert existing_al.get_strategy_object("uncertainty_sampling") is uncertainty.uncertainty_sampling
    assert existing_al.get_strategy_object("margin_sampling") is uncertainty.margin_sampling
    assert existing_al.get_strategy_object("entropy_sampling") is uncertainty.entropy_sampling


def test_surface_symbols_declared_exported_bound_and_marked_extension():
    header = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    assert re.search(r"\bsize_t\s+alink_kmeanspp_scratch_bytes\s*\(", header)
    assert re.search(r"\bint\s+alink_kmeanspp\s*\(", header)
    assert len(_abi.PROTOTYPES["alink_kmeanspp_scratch_bytes"][1]) == 2 and len(_abi.PROTOTYPES["alink_kmeanspp"][1]) == 13
    lib = _abi.load()
    assert hasattr(lib, "alink_kmeanspp") and hasattr(lib, "alink_kmeanspp_scratch_bytes")
    # two d2 buffers, two buffers of 2,048 float64 chunk sums, 2,048 (norm, index) candidates
    assert lib.alink_kmeanspp_scratch_bytes(1000, 4) == 2 * 4096 + 2 * 2048 * 8 + 2048 * 8
    assert lib.alink_kmeanspp_scratch_bytes(0, 4) == 0
    from a_link_amd import committee, head
    for obj in (badge, badge.kmeans_pp, badge.kmeans_pp_device, badge.badge_device, badge.badge_sampling, head.DenseHead.badge_device):
        assert "EXTENSION" in obj.__doc__, obj
    assert "X10" in badge.__doc__ and "Extension" in committee.Bagging.badge_indexed.__doc__


def test_no_kmeanspp_kernel_spills_to_scratch():
    """the build keeps hipcc's per-kernel resource report beside every object: no kernel of kmeanspp.hip may use scratch (the
    prologue's eight chunk sums and their cumulative sums per thread live in registers)"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "kmeanspp.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    seen, fn = 0, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            seen += 1
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
    assert seen >= 9, seen                                                  # norm and step in four forms each, and finish
