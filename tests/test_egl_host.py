"""CPU: expected gradient length and gradient embedding on the host (a-link_amd/egl.py) against a row-by-row loop over the
oracle's own gradients, saturated rows, the sampler, the new symbol's surface, and the egl kernels' scratch use."""
import os
import re

import numpy as np
import pytest

import a_link_amd  # noqa: F401
from a_link_amd import _abi, egl, uncertainty
from oracle import siamese_head as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(64, 128, 32, 2), (512, 512, 64, 2), (128, 384, 64, 1)]     # (D, h1, h2, od)
N = 70
SCALED = 6                                                             # the last rows, scaled by 64: saturated outputs
# seed per shape: the first at which, in the float64 oracle, every scaled row has 1 - max p below 1e-4 and at least three have
# it below 1e-9 (a scaled row whose two logits happen to meet is neither saturated nor a plain row: its logits are in the tens)
SEEDS = {(64, 128, 32, 2): 0, (512, 512, 64, 2): 2, (128, 384, 64, 1): 1, (520, 256, 64, 2): 1}


def make_case(D, h1, h2, od, n=N, seed=None):
    """weights (oracle.init_weights + small random biases) and n pairs, the last SCALED of them scaled by 64"""
    seed = SEEDS.get((D, h1, h2, od), 0) if seed is None else seed
    rng = np.random.RandomState(1000 + seed + D + h1 + h2 + od)
    ws = O.init_weights(D, h1, h2, seed=seed + 3, out_dim=od)
    for i in (1, 3, 5):
        ws[i] = (0.05 * rng.randn(*ws[i].shape)).astype(np.float32)
    L = rng.randn(n, D).astype(np.float32)
    R = rng.randn(n, D).astype(np.float32)
    L[n - SCALED:] *= 64
    R[n - SCALED:] *= 64
    return ws, L, R


def oracle_loop(ws, L, R):
    """row by row: EGL = sum_c P(c) |g_c| over the oracle's float64 gradients of the one-row batch, and gW3 for yhat
    -> (egl (N,), emb (N, od * h2) in the layout emb[c * h2 + j], p (N, od), smallest |z1| or |z2| of the row (N,))"""
    n = len(L)
    od = np.asarray(ws[4]).shape[1]
    p, (d, z1, a1, z2, a2) = O.forward(ws, L, R, dtype=np.float64, cache=True)
    out, emb = np.zeros(n), np.zeros((n, od * a2.shape[1]))
    for i in range(n):
        pi = p[i]
        prob = [pi[0], pi[1]] if od == 2 else [1 - pi[0], pi[0]]
        yhat = (1 if pi[1] > pi[0] else 0) if od == 2 else int(pi[0] > 0.5)
        for c in (0, 1):
            y = O.to_categorical([c]).astype(np.float64) if od == 2 else np.array([[float(c)]])
            gs, _, _ = O.gradients(ws, L[i:i + 1], R[i:i + 1], y, dtype=np.float64)
            out[i] += prob[c] * np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in gs))
            if c == yhat:
                emb[i] = gs[4].T.ravel()
    margin = np.minimum(np.abs(z1).min(axis=1), np.abs(z2).min(axis=1))
    return out, emb, p, margin


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "D%d_h%d_%d_od%d" % s)
def case(request):
    ws, L, R = make_case(*request.param)
    return (ws, L, R) + oracle_loop(ws, L, R)


def test_egl_matches_the_oracle_gradients(case):
    ws, L, R, ref, _, p, _ = case
    got = egl.expected_gradient_length(ws, [L, R])
    assert got.shape == (N,) and got.dtype == np.float64
    err = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    err[ref == 0] = np.abs(got[ref == 0])
    print("largest relative difference to the oracle loop: %.3g" % err.max())
    assert err.max() <= 1e-12
    assert (ref[:N - SCALED] > 0).all()                                # the unscaled rows are live


def test_gradient_embedding_matches_the_oracle_gW3(case):
    ws, L, R, _, ref, p, _ = case
    got = egl.gradient_embedding(ws, [L, R])
    assert got.shape == ref.shape and got.dtype == np.float64
    scale = np.abs(ref).max(axis=1, keepdims=True)
    live = scale[:, 0] > 0
    assert live[:N - SCALED].all()
    assert (np.abs(got - ref)[live] / scale[live]).max() <= 1e-12
    assert (got[~live] == 0).all()


def test_saturated_rows_are_exactly_zero(case):
    ws, L, R, ref, emb_ref, p, _ = case
    pmax = p.max(axis=1) if p.shape[1] == 2 else np.maximum(p[:, 0], 1 - p[:, 0])
    sat = np.flatnonzero(1 - pmax < 1e-9)
    assert len(sat) >= 2 and (sat >= N - SCALED).all()
    got, emb = egl.expected_gradient_length(ws, [L, R]), egl.gradient_embedding(ws, [L, R])
    assert (got[sat] == 0.0).all() and (emb[sat] == 0.0).all()
    assert (ref[sat] == 0.0).all()                                     # the train step's own gradient is zero there


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


def test_egl_sampling_returns_the_top_n_in_multi_argmax_order():
    ws, L, R = make_case(64, 128, 32, 2)
    values = egl.expected_gradient_length(ws, [L, R])
    for n in (1, 5, N):
        want = uncertainty.multi_argmax(values, n_instances=n)
        for clf in (_Learner(ws), _Estimator(ws), _Net(ws)):
            idx, inst = egl.egl_sampling(clf, [L, R], n_instances=n)
            assert np.array_equal(idx, want)
            assert np.array_equal(inst[0], L[want]) and np.array_equal(inst[1], L[want])
    idx, _ = egl.egl_sampling(_Net(ws), [L, R], n_instances=5)
    assert set(idx) == set(np.argsort(-values, kind="stable")[:5])
    with pytest.raises(TypeError):
        egl.egl_sampling(object(), [L, R])


def test_surface_symbol_declared_exported_bound_and_marked_extension():
    header = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    assert re.search(r"\bint\s+alink_head_egl\s*\(", header)
    assert "alink_head_egl" in _abi.PROTOTYPES and len(_abi.PROTOTYPES["alink_head_egl"][1]) == 12
    assert hasattr(_abi.load(), "alink_head_egl")
    from a_link_amd import committee, head
    for obj in (egl, egl.expected_gradient_length, egl.gradient_embedding, egl.egl_sampling, egl.expected_gradient_length_device,
                head.DenseHead.expected_gradient_length_device):
        assert "EXTENSION" in obj.__doc__, obj
    assert "X9" in egl.__doc__ and "Extension" in committee.Bagging.egl_indexed.__doc__


def test_no_egl_kernel_spills_to_scratch():
    """the build keeps hipcc's per-kernel resource report beside every object: no instantiation of head_egl_kernel may use
    scratch (three GEMMs' accumulators and the mask live in registers across the whole kernel)"""
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "egl.usage")
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
