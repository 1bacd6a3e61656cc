"""CPU: ALFA-Mix on the host (a-link_amd/alfamix.py) — the mix direction against torch's float64 autograd, the geometry of the
mixed rows, the batch rule on hand-set masks, the sampler and the strategy name, the new symbol's surface, and the mix kernels'
scratch use."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import a_link_amd  # noqa: F401
from a_link_amd import _abi, alfamix, cluster
from test_egl_host import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(64, 128, 32, 2), (512, 512, 64, 2), (128, 384, 64, 1), (8, 128, 32, 2), (504, 256, 64, 2)]     # (D, h1, h2, od)
IDS = ["D%d_h%d_%d_od%d" % s for s in SHAPES]
N = 70
# (eps, rows of the 70 that flip under some anchor in float64): the eps at which a shape has rows of both kinds
FLIPPING = {(64, 128, 32, 2): (0.1, 26), (512, 512, 64, 2): (0.1, 52), (504, 256, 64, 2): (0.1, 42), (128, 384, 64, 1): (0.5, 43)}


def labelled_anchors(ws, D):
    """40 labelled rows, labelled by the float64 head's own prediction -> (rows float32 (40, D), y (40,), anchors (3, D)): the two
    class means (the mean of all rows standing in for an empty class) and a third anchor of zeros"""
    rng = np.random.RandomState(7)
    Ld = np.abs(rng.randn(40, D) - rng.randn(40, D)).astype(np.float32)
    p = alfamix.feature_mix(ws, [Ld, np.zeros_like(Ld)], np.zeros((1, D), np.float32), eps=0.0)["probs"]
    y = alfamix._argmax(p)
    rows = Ld.astype(np.float64)
    means = [rows[y == c].mean(axis=0) if (y == c).any() else rows.mean(axis=0) for c in (0, 1)]
    return Ld, y, np.stack(means + [np.zeros(D)]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(shape):
    ws, L, R = make_case(*shape)
    Ld, y, anchors = labelled_anchors(ws, shape[0])
    for a in (L, R, Ld, y, anchors):
        a.setflags(write=False)
    return ws, L, R, Ld, y, anchors


def autograd_direction(ws, L, R, yhat):
    """torch float64 autograd of the predicted class's negative margin with respect to d = |l - r|"""
    W1, b1, W2, b2, W3, b3 = [torch.from_numpy(np.asarray(w, np.float64)) for w in ws]
    d = torch.from_numpy(np.abs(L.astype(np.float64) - R.astype(np.float64))).requires_grad_(True)
    z3 = torch.relu(torch.relu(d @ W1 + b1) @ W2 + b2) @ W3 + b3
    yh = torch.from_numpy(yhat)
    if z3.shape[1] == 2:
        margin = torch.where(yh == 1, z3[:, 1] - z3[:, 0], z3[:, 0] - z3[:, 1])
    else:
        margin = torch.where(yh == 1, z3[:, 0], -z3[:, 0])
    (-margin).sum().backward()
    return d.grad.numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_direction_is_the_autograd_gradient_of_the_negative_margin(shape):
    ws, L, R, _, _, anchors = case(shape)
    out = alfamix.feature_mix(ws, [L, R], anchors, eps=0.2)
    assert out["g"].shape == (N, shape[0]) and out["g"].dtype == np.float64
    ref = autograd_direction(ws, L, R, out["yhat"])
    top = np.abs(ref).max(axis=1)
    assert (top > 0).all()
    err = float((np.abs(out["g"] - ref).max(axis=1) / top).max())
    print("%s: largest row-wise relative difference to autograd %.3g" % (shape, err))
    assert err <= 1e-12


@pytest.mark.parametrize("eps", [0.1, 0.2, 0.5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_mixed_rows_lie_between_the_row_and_the_anchor_within_the_step(shape, eps):
    ws, L, R, _, _, anchors = case(shape)
    out = alfamix.feature_mix(ws, [L, R], anchors, eps=eps)
    d = np.abs(L.astype(np.float64) - R.astype(np.float64))
    assert out["mixed"].shape == (N, 3, shape[0]) and out["mixed_probs"].shape == (N, 3, shape[3]) and out["margin"].shape == (N, 3)
    assert out["flip"].dtype == np.uint8 and out["flip"].shape == (N,) and (out["flip"] < 8).all()
    for a in range(3):
        an = anchors[a].astype(np.float64)[None, :]
        m = out["mixed"][:, a]
        slack = 4 * np.spacing(np.maximum(np.abs(d), np.abs(an)))                 # d + (an - d) rounds twice
        assert (m >= np.minimum(d, an) - slack).all() and (m <= np.maximum(d, an) + slack).all()
        z = an - d
        step = np.sqrt(((m - d) ** 2).sum(axis=1))
        assert (step <= eps * np.sqrt((z * z).sum(axis=1)) * (1 + 1e-9)).all()
        # the flip bit is the argmax rule on the mixed probabilities, and agrees with the sign of the mixed margin
        flipped = alfamix._argmax(out["mixed_probs"][:, a]) != out["yhat"]
        assert np.array_equal((out["flip"] >> a & 1).astype(bool), flipped)
        assert (out["margin"][:, a][flipped] <= 0).all() and (out["margin"][:, a][~flipped] >= 0).all()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_that_flip_and_rows_that_do_not(shape):
    """the conditions the device test relies on: at its eps a shape has rows that flip and rows that do not under EVERY anchor;
    (8, 128, 32, 2) flips nothing up to eps = 0.5; the one-output shape at eps = 0.2 has 3 candidates (the fill case)"""
    ws, L, R, _, _, anchors = case(shape)
    if shape not in FLIPPING:
        assert not alfamix.feature_mix(ws, [L, R], anchors, eps=0.5)["flip"].any()
        return
    eps, count = FLIPPING[shape]
    flip = alfamix.feature_mix(ws, [L, R], anchors, eps=eps)["flip"]
    print("%s eps=%g: %d of %d rows flip under some anchor" % (shape, eps, (flip != 0).sum(), N))
    assert (flip != 0).sum() == count
    for a in range(3):
        bit = flip >> a & 1
        assert 0 < bit.sum() < N, (a, bit.sum())
    if shape[3] == 1:
        assert (alfamix.feature_mix(ws, [L, R], anchors, eps=0.2)["flip"] != 0).sum() == 3


def test_eps_zero_flips_nothing_and_dead_rows_do_not_move():
    shape = SHAPES[0]
    ws, L, R, _, _, anchors = case(shape)
    d = np.abs(L.astype(np.float64) - R.astype(np.float64))
    out = alfamix.feature_mix(ws, [L, R], anchors, eps=0.0)
    assert not out["flip"].any() and np.array_equal(out["mixed"], np.repeat(d[:, None, :], 3, axis=1))
    dead = [np.array(w) for w in ws]
    dead[1] = np.full_like(dead[1], -1e6)                                          # every first-layer unit is off on every row
    out = alfamix.feature_mix(dead, [L, R], anchors, eps=0.5)
    assert (out["g"] == 0).all() and np.array_equal(out["mixed"], np.repeat(d[:, None, :], 3, axis=1)) and not out["flip"].any()
    with pytest.raises(ValueError, match="eps"):
        alfamix.feature_mix(ws, [L, R], anchors, eps=-0.1)
    with pytest.raises(ValueError, match="eps"):
        alfamix.feature_mix(ws, [L, R], anchors, eps=float("nan"))
    with pytest.raises(ValueError, match="anchors"):
        alfamix.feature_mix(ws, [L, R], np.zeros((9, shape[0]), np.float32))
    with pytest.raises(ValueError, match="anchors"):
        alfamix.feature_mix(ws, [L, R], np.zeros((2, shape[0] + 8), np.float32))


def test_class_anchors():
    rows = np.array([[0, 0], [2, 4], [4, 8], [1, 1]], np.float32)
    got = alfamix.class_anchors(rows, [0, 1, 1, 0])
    assert got.dtype == np.float32 and np.array_equal(got, np.array([[0.5, 0.5], [3, 6]], np.float32))
    assert np.array_equal(alfamix.class_anchors(rows, np.eye(2)[[0, 1, 1, 0]]), got)           # one-hot labels
    assert np.array_equal(alfamix.class_anchors(rows, np.array([[0.], [1.], [1.], [0.]])), got)
    assert np.array_equal(alfamix.class_anchors([rows, np.zeros_like(rows)], [0, 1, 1, 0]), got)  # pair input: |l - r|
    assert np.array_equal(alfamix.class_anchors(rows, [1, 1, 1, 1]), rows.mean(axis=0, keepdims=True))   # an empty class: no anchor
    third = np.float32(1) / np.float32(3)
    one = alfamix.class_anchors(np.array([[third], [third], [1.0]], np.float32), [0, 0, 0])
    assert one[0, 0] == np.float32((np.float64(third) * 2 + 1) / 3)                # the mean in float64, rounded once
    with pytest.raises(ValueError):
        alfamix.class_anchors(rows, [0, 1])


def _pool():
    """12 rows in three well-separated groups of four, probabilities that order the fill, ties included"""
    rows = np.array([[0, 0], [0, 1], [1, 0], [1, 1], [20, 0], [20, 1], [21, 0], [21, 1], [0, 20], [0, 21], [1, 20], [1, 21]], np.float64)
    p0 = np.array([.9, .8, .55, .7, .6, .55, .95, .5, .45, .3, .2, .1], np.float32)
    return rows, np.stack([p0, 1 - p0], axis=1)


def test_select_with_enough_candidates_is_one_query_per_cluster():
    rows, probs = _pool()
    flip = np.zeros(12, np.uint8)
    cand = np.array([0, 3, 4, 5, 7, 9, 10])
    flip[cand] = [1, 2, 4, 1, 3, 7, 1]
    picks = alfamix.select(rows, flip, probs, 3, iters=5, random_state=0)
    assert picks.dtype == np.int64 and len(picks) == 3 and len(set(picks)) == 3 and set(picks) <= set(cand)
    assert sorted(p // 4 for p in picks) == [0, 1, 2]                              # one per group
    near = cluster._host_pick(rows[cand], 3, 5, 0)
    assert np.array_equal(picks, cand[near])
    assert set(alfamix.select(rows, flip, probs, 7, random_state=1)) == set(cand)  # as many clusters as candidates: all of them


def test_select_with_too_few_candidates_fills_by_smallest_margin():
    rows, probs = _pool()
    flip = np.zeros(12, np.uint8)
    flip[[6, 2]] = 1
    picks = alfamix.select(rows, flip, probs, 5)
    # |p0 - p1|: row 7 is 0, rows 2, 5 and 8 tie at 0.1 (2 is picked already): the lower index first
    value = np.abs(probs[:, 0] - probs[:, 1])
    assert value[5] == value[8] == value[2]
    assert picks.tolist() == [2, 6, 7, 5, 8]
    assert alfamix.select(rows, np.zeros(12, np.uint8), probs, 2).tolist() == [7, 2]                # no candidate at all
    one = probs[:, :1].copy()                                                      # one output: |2p - 1|
    assert alfamix.select(rows, np.zeros(12, np.uint8), one, 2).tolist() == [7, 2]
    assert len(alfamix.select(rows, flip, probs, 50)) == 12                        # clipped to the pool


def test_select_fills_for_an_empty_cluster():
    rows, probs = _pool()
    rows = rows.copy()
    rows[[1, 2, 3]] = rows[0]                                                      # four candidates, two distinct rows
    flip = np.zeros(12, np.uint8)
    flip[[0, 1, 2, 4]] = 1
    picks = alfamix.select(rows, flip, probs, 3, random_state=0)
    assert len(picks) == 3 and len(set(picks)) == 3
    assert set(picks[:2]) <= {0, 1, 2, 4} and 4 in picks[:2]                        # two clusters have rows, the third stays empty
    rest = [i for i in np.argsort(np.abs(probs[:, 0] - probs[:, 1]), kind="stable") if i not in picks[:2]]
    assert picks[2] == rest[0] == 7


def test_select_never_picks_an_excluded_row():
    rows, probs = _pool()
    flip = np.zeros(12, np.uint8)
    flip[[6, 2, 7]] = 1
    picks = alfamix.select(rows, flip, probs, 4, exclude=[7, 5])
    assert picks.tolist() == [2, 6, 8, 4]                                          # 7 (a candidate) and 5 (the best fill) are left out
    picks = alfamix.select(rows, flip, probs, 2, exclude=[7])
    assert set(picks) == {2, 6}
    assert len(alfamix.select(rows, flip, probs, 50, exclude=[0, 1])) == 10
    with pytest.raises(ValueError):
        alfamix.select(rows, flip, probs, 1, exclude=list(range(12)))
    with pytest.raises(ValueError):
        alfamix.select(rows, flip[:5], probs, 1)
    with pytest.raises(ValueError):
        alfamix.select(rows, flip, probs, 0)


class _Net(object):
    def __init__(self, ws):
        self.ws = ws

    def get_weights(self):
        return self.ws


class _Estimator(object):
    def __init__(self, ws):
        self.siamese_net = _Net(ws)


class _Learner(object):
    def __init__(self, ws, X_training=None, y_training=None):
        self.estimator = _Estimator(ws)
        self.X_training, self.y_training = X_training, y_training


def test_sampler_and_strategy_name():
    from a_link_amd import existing_al
    shape = SHAPES[0]
    ws, L, R, Ld, y, _ = case(shape)
    assert existing_al.get_strategy_object("alfamix_sampling") is alfamix.alfamix_sampling
    training = [Ld, np.zeros_like(Ld)]
    learner = _Learner(ws, training, y)
    idx, inst = alfamix.alfamix_sampling(learner, [L, R], n_instances=6, eps=0.1, random_state=3)
    anchors = alfamix.class_anchors(training, y)
    want, info = alfamix.alfamix(ws, [L, R], anchors, 6, eps=0.1, random_state=3)
    assert np.array_equal(idx, want) and len(set(idx)) == 6
    assert (info["flip"][idx] != 0).all()                                          # 26 candidates: every pick is one
    assert np.array_equal(inst[0], L[idx]) and np.array_equal(inst[1], L[idx])
    idx1, _ = alfamix.alfamix_sampling(learner, [L, R])
    assert len(idx1) == 1
    with pytest.raises(ValueError, match="labelled"):
        alfamix.alfamix_sampling(_Learner(ws), [L, R])
    with pytest.raises(TypeError):
        alfamix.alfamix_sampling(object.__new__(type("Bare", (), {"X_training": training, "y_training": y})), [L, R])


def test_surface_symbol_declared_exported_bound_and_marked_extension():
    header = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    assert re.search(r"\bint\s+alink_head_feature_mix\s*\(", header)
    assert "alink_head_feature_mix" in _abi.PROTOTYPES and len(_abi.PROTOTYPES["alink_head_feature_mix"][1]) == 14
    assert hasattr(_abi.load(), "alink_head_feature_mix")
    from a_link_amd import committee, head
    for obj in (alfamix, alfamix.class_anchors, alfamix.feature_mix, alfamix.select, alfamix.alfamix, alfamix.feature_mix_device,
                alfamix.select_device, alfamix.alfamix_device, alfamix.alfamix_sampling, head.DenseHead.feature_mix_device):
        assert "EXTENSION" in obj.__doc__, obj
    assert "X15" in alfamix.__doc__ and "Extension" in committee.Bagging.alfamix_indexed.__doc__
    assert "synchronisation" in alfamix.alfamix_device.__doc__


def test_no_mix_kernel_spills_to_scratch():
    """the build keeps hipcc's per-kernel resource report beside every object: no instantiation of head_mix_kernel may use scratch
    (layer 1's accumulators and the input gradient live in registers across the anchors)"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "alfamix.usage")
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
    assert seen >= 4, seen
