"""CPU: BAIT's host rule (a_link_amd/bait.py) — the rank-one reduction against the paper's general trace
expression, the Woodbury state, the block (committee) form, the shape of the result, and the plumbing."""
import os
import re

import numpy as np
import pytest

import a_link_amd  # noqa: F401
from a_link_amd import _abi, bait, egl
from test_egl_host import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200
LAB = np.arange(20)


def head_case(od, seed=0):
    """a random 32/64/64/od head and N pairs; make_case scales its last rows by 64, so a few rows saturate"""
    return make_case(32, 64, 64, od, n=N, seed=seed)


def general_V(ws, X):
    """the paper's per-sample factor V_x (2 rows over the last layer's weights): row c = sqrt(P(c | x)) grad l(x, c), so that
    V_x^T V_x is the sample's Fisher.  Saturated rows are zero, as the package's rule has them.  -> (N, 2, od h2) float64"""
    p, _, _, _, a2, _, _, _ = egl._host_pass(ws, X)
    od, h2 = p.shape[1], a2.shape[1]
    V = np.zeros((len(p), 2, od * h2))
    for c in (0, 1):
        if od == 2:
            dz = p.copy()
            dz[:, c] -= 1.0                                                 # softmax + cross-entropy: dz = p - e_c
            pc = p[:, c]
        else:
            dz = p - float(c)                                               # sigmoid + cross-entropy: dz = p - y
            pc = p[:, 0] if c == 1 else 1 - p[:, 0]
        g = (dz[:, :, None] * a2[:, None, :]).reshape(len(p), od * h2)
        V[:, c] = np.sqrt(pc)[:, None] * g
    V[~egl._inside(p)] = 0.0
    return V


@pytest.mark.parametrize("od", [2, 1])
def test_rank_one_score_equals_the_papers_trace_expression(od):
    ws, L, R = head_case(od)
    X = [L, R]
    V = general_V(ws, X)
    G = V.shape[2]
    lam = 1.0
    Phi = np.einsum("nci,ncj->ij", V, V) / N
    M = lam * np.eye(G) + np.einsum("nci,ncj->ij", V[LAB], V[LAB])
    Bg = np.linalg.inv(M)
    Ag = Bg @ Phi @ Bg
    want = np.array([np.trace(v @ Ag @ v.T @ np.linalg.inv(np.eye(2) + v @ Bg @ v.T)) for v in V])
    f = bait.fisher_factor(ws, X)
    assert f.shape == (N, 64)
    phi = bait.fisher_matrix(f, scale=1.0 / N)
    B = np.linalg.inv(lam * np.eye(64)[None] + bait.fisher_matrix(f, rows=LAB))
    got = bait.bait_scores(f, B @ phi @ B, B)
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("od = %d: rank-one score against the general expression, relative %.2e" % (od, rel))
    assert rel < 1e-10
    sat = ~egl._inside(egl._host_pass(ws, X)[0])
    assert (f[sat] == 0).all() and (got[sat] == 0).all()


def _problem(seed=3, n=600, F=16, m=1, n_lab=12):
    rng = np.random.RandomState(seed)
    f = rng.randn(n, m * F) * rng.rand(n, 1)
    lab = rng.choice(n, n_lab, replace=False)
    free = np.ones(n, bool)
    free[lab] = False
    phi = bait.fisher_matrix(f, scale=1.0 / n, blocks=m)
    M0 = np.eye(F)[None] + bait.fisher_matrix(f, rows=lab, blocks=m)
    return f, lab, free, phi, M0


def test_running_inverse_after_forward_and_backward_steps():
    """128 forward and 64 backward rank-one steps: the running B against a fresh inverse"""
    f, lab, free, phi, M0 = _problem(n=600, F=16)
    idx, B = bait.bait_select(f, phi, M0, 64, over=2, free=free)
    assert len(idx) == 64
    want = np.linalg.inv(M0[0] + f[idx].T @ f[idx])
    rel = np.abs(B[0] - want).max() / np.abs(want).max()
    print("running inverse against np.linalg.inv after 128 + 64 steps: %.2e" % rel)
    assert rel < 1e-10


def test_block_form_is_the_sum_of_the_members_scores():
    f, lab, free, phi, M0 = _problem(F=16, m=2)
    B = np.linalg.inv(M0)
    A = B @ phi @ B
    both = bait.bait_scores(f, A, B, blocks=2)
    one = bait.bait_scores(f[:, :16], A[:1], B[:1]) + bait.bait_scores(f[:, 16:], A[1:], B[1:])
    assert np.allclose(both, one, rtol=1e-13, atol=0)
    back = bait.bait_scores(f, A, B, sign=-1, blocks=2)
    qb = [np.einsum("ni,ij,nj->n", f[:, j * 16:(j + 1) * 16], B[j], f[:, j * 16:(j + 1) * 16]) for j in (0, 1)]
    skip = (qb[0] >= 1) | (qb[1] >= 1)
    assert np.isnan(back[skip]).all() and not np.isnan(back[~skip]).any() and (back[~skip] <= 0).all()
    idx, Bout = bait.bait_select(f, phi, M0, 10, blocks=2, free=free)
    assert len(set(idx)) == 10 and Bout.shape == (2, 16, 16)
    for j in (0, 1):
        fj = f[idx, j * 16:(j + 1) * 16]
        assert np.allclose(Bout[j], np.linalg.inv(M0[j] + fj.T @ fj), rtol=0, atol=1e-10)


def test_result_shape():
    f, lab, free, phi, M0 = _problem()
    k = 20
    idx, B = bait.bait_select(f, phi, M0, k, free=free)
    assert idx.dtype == np.int64 and len(idx) == k and len(set(idx)) == k and not set(idx) & set(lab)
    first = np.flatnonzero(free)[:k]
    naive = np.trace(np.linalg.inv(M0[0] + f[first].T @ f[first]) @ phi[0])
    assert np.trace(B[0] @ phi[0]) <= naive
    # the prune only removes what the forward phase picked, and keeps the order of the picks
    fwd, _ = bait.bait_select(f, phi, M0, 2 * k, over=1, free=free)
    assert [n for n in fwd if n in set(idx)] == list(idx)
    # fewer free rows than asked for: all of them
    few = np.zeros(len(f), bool)
    few[[5, 9, 11]] = True
    assert sorted(bait.bait_select(f, phi, M0, 8, free=few)[0]) == [5, 9, 11]


def test_identical_rows_are_picked_in_index_order():
    f = np.tile(np.linspace(0.1, 0.8, 8), (40, 1))
    phi = bait.fisher_matrix(f, scale=1.0 / 40)
    M0 = np.eye(8)[None]
    assert list(bait.bait_select(f, phi, M0, 6, over=1)[0]) == [0, 1, 2, 3, 4, 5]
    # with the prune: 12 forward picks 0 .. 11, and of equal scores the EARLIER pick is removed
    assert list(bait.bait_select(f, phi, M0, 6)[0]) == [6, 7, 8, 9, 10, 11]


class _Net(object):
    def __init__(self, ws):
        self.ws = ws

    def get_weights(self):
        return self.ws


class _Estimator(object):
    def __init__(self, ws):
        self.siamese_net = _Net(ws)


def test_sampler_through_the_learner_and_strategy_name():
    from a_link_amd import existing_al
    from a_link_amd.learners import ActiveLearner
    assert existing_al.get_strategy_object("bait_sampling") is bait.bait_sampling
    assert "bait_sampling" in existing_al.get_strategy_object.__doc__
    ws, L, R = head_case(2)
    learner = ActiveLearner(estimator=_Estimator(ws), query_strategy=bait.bait_sampling)
    idx, inst = learner.query([L, R], n_instances=7)
    want = bait.bait(ws, [L, R], None, 7)
    assert np.array_equal(idx, want) and len(set(idx)) == 7
    assert np.array_equal(inst[0], L[idx]) and np.array_equal(inst[1], L[idx])
    assert len(bait.bait_sampling(_Net(ws), [L, R])[0]) == 1
    with_lab = bait.bait(ws, [L, R], LAB, 7)
    assert len(set(with_lab)) == 7 and not set(with_lab) & set(LAB)
    with pytest.raises(TypeError):
        bait.bait_sampling(object(), [L, R])


def test_argument_errors():
    f, lab, free, phi, M0 = _problem()
    with pytest.raises(ValueError):
        bait.bait_select(f, phi, M0, 0)
    with pytest.raises(ValueError):
        bait.bait_select(f, phi, M0, 4, over=0)
    with pytest.raises(ValueError):
        bait.bait_select(f, phi, M0, 4, free=np.zeros(len(f), bool))
    with pytest.raises(ValueError):
        bait.bait_select(f, phi, M0, 4, free=np.ones(3, bool))
    with pytest.raises(ValueError):
        bait.bait_select(f, phi, M0, 4, blocks=3)                              # 16 columns are not three blocks
    ws, L, R = head_case(2)
    with pytest.raises(ValueError):
        bait.bait(ws, [L, R], [0, 0], 4)
    with pytest.raises(ValueError):
        bait.bait(ws, [L, R], [N], 4)
    for F, m in ((12, 1), (136, 1), (128, 5), (8, 9), (0, 1)):
        with pytest.raises(ValueError):
            bait._check_shape(F, m)
    bait._check_shape(128, 4)
    bait._check_shape(8, 8)


def test_first_argmax_ties_nan_and_minus_infinity():
    inf, nan = np.inf, np.nan
    assert bait.first_argmax(np.array([1.0, 3.0, 3.0, nan]), np.ones(4, bool)) == 1
    assert bait.first_argmax(np.array([1.0, 3.0, 3.0, nan]), np.array([1, 0, 1, 1], bool)) == 2
    assert bait.first_argmax(np.array([nan, -inf, -inf]), np.ones(3, bool)) == 1       # -inf is a score: it can win, as on the device
    assert bait.first_argmax(np.array([nan, nan]), np.ones(2, bool)) == -1
    assert bait.first_argmax(np.array([1.0, 2.0]), np.zeros(2, bool)) == -1


def test_saturated_rows_have_zero_factors_and_are_picked_by_index():
    ws, L, R = head_case(2)
    ws = [w.copy() for w in ws]
    ws[5] = ws[5] + np.array([60.0, -60.0], np.float32)                       # every row saturates
    f = bait.fisher_factor(ws, [L, R])
    assert (f == 0).all()
    assert list(bait.bait(ws, [L, R], None, 5, over=1)) == [0, 1, 2, 3, 4]
    assert list(bait.bait(ws, [L, R], [0, 2], 3, over=1)) == [1, 3, 4]
    assert list(bait.bait_sampling(_Net(ws), [L, R], n_instances=5)[0]) == [5, 6, 7, 8, 9]    # 10 picks, the earlier of equals pruned


def test_factor_rule_from_the_heads_outputs():
    """the device's rule (emb of the other class x a scale of the probabilities) restated in NumPy gives the ideal factor"""
    for od in (2, 1):
        ws, L, R = head_case(od)
        p = egl._host_pass(ws, [L, R])[0]
        emb = egl.gradient_embedding(ws, [L, R])
        got = bait.factor_from_outputs(p, emb)
        want = bait.fisher_factor(ws, [L, R])
        # the scale is rounded to float32 once: 6e-8 relative
        assert np.abs(got - want).max() <= 1.2e-7 * np.abs(want).max()
        assert (got[~egl._inside(p)] == 0).all()


def test_pack_ab_layout():
    F = 16
    A = np.arange(F * F, dtype=np.float64).reshape(1, F, F)
    img = bait.pack_ab(A, -A)
    assert img.shape == (1, 2, F * F) and img.dtype == np.float32
    for k, c in ((0, 0), (1, 0), (2, 5), (7, 15), (8, 3), (15, 15)):
        at = ((k // 8) * F + c) * 8 + (k % 2) * 4 + (k % 8) // 2
        assert img[0, 0, at] == A[0, k, c] and img[0, 1, at] == -A[0, k, c]


def test_surface_declared_bound_and_marked_extension():
    header = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    lib = _abi.load()
    for name in ("alink_fisher_factor", "alink_bait_scores", "alink_bait_select", "alink_bait_select_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _abi.PROTOTYPES and hasattr(lib, name)
    assert "X16" in header and "X16" in bait.__doc__
    m = re.search(r"#define ALINK_BAIT_TILE (\d+)", header)
    assert m and int(m.group(1)) == bait.TILE
    from a_link_amd import committee, head
    for obj in (bait, bait.fisher_factor, bait.fisher_matrix, bait.bait_select, bait.bait, bait.fisher_factor_device,
                bait.bait_select_device, bait.bait_device, bait.bait_sampling, head.DenseHead.bait_device):
        assert "EXTENSION" in obj.__doc__, obj
    assert "Extension" in committee.Bagging.bait_indexed.__doc__
    assert "synchronisation" in bait.bait_select_device.__doc__


def test_no_bait_kernel_spills_to_scratch():
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "bait.usage")
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
    assert seen >= 8, seen
