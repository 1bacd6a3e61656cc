"""GPU: ranked batch-mode selection on device (alink_ranked_batch, batch.hip) — bit equality with a float32 NumPy emulation of
the rule on inputs that admit no rounding, the float64 maximum within a derived bound on real-valued features, the pair form
against the row form, position independence, ties, what the rule is for, fixed alpha, and Bagging.ranked_batch_indexed."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


# ---- the rule of include/alink_hip.h in NumPy ---------------------------------------------------------------------------------
def _emulate(X, Z, u, k, alpha=None, dtype=np.float32):
    """picks and scores of the rule, every operation rounded to `dtype`.  The squared distances are NumPy row sums: exact — so
    order-free — on the integer inputs the bit-equality tests use."""
    X, Z, u = X.astype(dtype), Z.astype(dtype), u.astype(dtype)
    N, M = len(X), len(Z)
    one = dtype(1)
    d2 = np.full(N, np.inf, dtype)
    for z in Z:
        d2 = np.minimum(d2, ((X - z) ** 2).sum(axis=1, dtype=dtype))
    picked = np.zeros(N, bool)
    idx, scores = [], []
    for t in range(min(k, N)):
        a = dtype(np.float64(N - t) / np.float64(N + M)) if alpha is None else dtype(alpha)
        s = one / (one + np.sqrt(d2))
        score = a * (one - s) + (one - a) * u
        score[picked] = -np.inf
        cand = np.flatnonzero(~picked)
        p = int(cand[np.argmax(score[cand])])                                # the first maximum among the rows left
        idx.append(p)
        scores.append(score[p])
        picked[p] = True
        d2 = np.minimum(d2, ((X - X[p]) ** 2).sum(axis=1, dtype=dtype))
    return np.array(idx, np.int32), np.array(scores, dtype)


def _run(rows, u, Z, k, alpha=None):
    from a_link_amd import batch as B
    if isinstance(rows, tuple):
        dev_rows = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in rows)
    else:
        dev_rows = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    idx, sc = B.ranked_batch_device(dev_rows, torch.from_numpy(u).cuda(), torch.from_numpy(Z).cuda(), k, alpha=alpha)
    assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and idx.is_cuda and sc.is_cuda
    return idx.cpu().numpy(), sc.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _integer_case(N, D, M, seed):
    """features in [-8, 8]: D * 16^2 < 2^24, every squared distance exact in float32 in any order; utilities in [0, 1)"""
    rng = np.random.RandomState(seed)
    X = rng.randint(-8, 9, (N, D)).astype(np.float32)
    Z = rng.randint(-8, 9, (M, D)).astype(np.float32)
    return X, Z, rng.rand(N).astype(np.float32)


def _pair_tables(rng, N, D, integer):
    nl, nr = 37, 11
    if integer:                                                              # in [-4, 4]: |l - r| in [0, 8]
        L, R = rng.randint(-4, 5, (nl, D)).astype(np.float32), rng.randint(-4, 5, (nr, D)).astype(np.float32)
    else:
        L, R = _unit(rng.randn(nl, D)), _unit(rng.randn(nr, D))
    li, ri = rng.randint(0, nl, N).astype(np.int32), rng.randint(0, nr, N).astype(np.int32)
    return L, R, li, ri


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _real_case(N, D, M, seed):
    """rows |a - b| of unit-norm vectors, utilities in [0, 1)"""
    rng = np.random.RandomState(seed)
    X = np.abs(_unit(rng.randn(N, D)) - _unit(rng.randn(N, D)))
    Z = np.abs(_unit(rng.randn(M, D)) - _unit(rng.randn(M, D)))
    return X, Z, rng.rand(N).astype(np.float32)


# (N, D, M, k): N off the wave's two rows and the workgroup's eight, D off 4 and off the 256-element lane sweep, D > 256 (a
# second sweep), a pool exhausted, one row, k beyond N; then the paths the kernels add: M beyond one LDS tile of labelled rows
# (16 rows at D = 512, the last tile partly filled), D > 512 (the init kernel's any-D form: 13-row tiles, three sweeps) and N
# beyond one sweep of the 2,048-workgroup grid (16,384 rows)
SHAPES = [(777, 40, 5, 64), (1031, 512, 3, 64), (300, 7, 1, 300), (1, 5, 1, 1), (4, 6, 2, 10), (515, 512, 37, 8), (130, 600, 31, 8),
          (16391, 12, 2, 8)]


@pytest.mark.parametrize("N,D,M,k", SHAPES)
def test_bit_equal_to_the_float32_emulation(gpu, N, D, M, k):
    X, Z, u = _integer_case(N, D, M, 100 + N)
    want_idx, want_sc = _emulate(X, Z, u, k)
    idx, sc = _run(X, u, Z, k)
    assert idx.shape == (min(k, N),) and sc.shape == (min(k, N),)
    assert np.array_equal(idx, want_idx)
    assert np.array_equal(_bits(sc), _bits(want_sc))
    if (N, D) == (777, 40):                                                  # the distance term is at work: not the plain top-k
        assert len(set(want_idx.tolist()) - set(np.argsort(-u, kind="stable")[:k].tolist())) == 5


@pytest.mark.parametrize("N,D", [(1003, 512), (1003, 40)])
def test_real_valued_picks_hold_the_float64_maximum(gpu, N, D):
    """Replay the device's picks in float64: at every step the device's pick scores within 2e of the float64 maximum, and the
    score it reports is within e of the float64 score, e = ((D + 4) / 4 + 6) 2^-24 — a D-term sum of squares carries at most
    (D + 2) 2^-24 relative error, the square root halves it, |d(1 / (1 + d))| <= 1/4 of d's relative error, a few unit
    roundoffs for the rest; utilities in [0, 1].  Largest gap seen on the MI355X: 0 at both sizes (the picks are the float64
    picks); largest score error 8.4e-8 at D = 512, 1.0e-7 at D = 40."""
    M, k = 7, 64
    X, Z, u = _real_case(N, D, M, 7 + D)
    idx, sc = _run(X, u, Z, k)
    e = ((D + 4) / 4.0 + 6.0) * 2.0 ** -24
    X64, u64 = X.astype(np.float64), u.astype(np.float64)
    d2 = ((X64[:, None, :] - Z.astype(np.float64)[None, :, :]) ** 2).sum(axis=2).min(axis=1)
    picked = np.zeros(N, bool)
    gap_max = err_max = 0.0
    for t, p in enumerate(idx):
        assert 0 <= p < N and not picked[p]
        a = float(np.float32(np.float64(N - t) / np.float64(N + M)))
        score = a * (1.0 - 1.0 / (1.0 + np.sqrt(d2))) + (1.0 - a) * u64
        gap_max = max(gap_max, float(score[~picked].max() - score[p]))
        err_max = max(err_max, abs(float(sc[t]) - float(score[p])))
        picked[p] = True
        d2 = np.minimum(d2, ((X64 - X64[p]) ** 2).sum(axis=1))
    print("D=%d: largest gap to the float64 maximum %.3e, largest |device score - float64 score| %.3e (e = %.3e)" % (D, gap_max, err_max, e))
    assert gap_max <= 2 * e, gap_max
    assert err_max <= e, err_max


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D, integer):
    """row n = |L[li[n]] - R[ri[n]]| formed on the fly == the row form on the materialised rows, bit for bit: one summation
    order for both.  D = 7 runs the scalar loads."""
    N, M, k = 1001, 4, 48
    rng = np.random.RandomState(3 * D + integer)
    L, R, li, ri = _pair_tables(rng, N, D, integer)
    rows = np.abs(L[li] - R[ri])
    Z = rows[rng.randint(0, N, M)] + (1.0 if integer else 0.01)
    u = rng.rand(N).astype(np.float32)
    idx_r, sc_r = _run(rows, u, Z, k)
    idx_p, sc_p = _run((L, R, li, ri), u, Z, k)
    assert np.array_equal(idx_p, idx_r)
    assert np.array_equal(_bits(sc_p), _bits(sc_r))
    if integer:
        want_idx, want_sc = _emulate(rows, Z, u, k)
        assert np.array_equal(idx_p, want_idx) and np.array_equal(_bits(sc_p), _bits(want_sc))


def test_rows_off_the_vector_alignment(gpu):
    """a row table 4 bytes off a 16-byte boundary takes the scalar loads: same bits"""
    from a_link_amd import batch as B
    X, Z, u = _real_case(300, 40, 3, 11)
    want = _run(X, u, Z, 32)
    flat = torch.empty(300 * 40 + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(300, 40)
    view.copy_(torch.from_numpy(X))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    idx, sc = B.ranked_batch_device(view, torch.from_numpy(u).cuda(), torch.from_numpy(Z).cuda(), 32)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(_bits(sc.cpu().numpy()), _bits(want[1]))


def test_position_independence(gpu):
    """a permutation of the pool rows (real-valued: no ties) permutes the picks and leaves the scores bit-equal"""
    X, Z, u = _real_case(1003, 40, 7, 21)
    idx, sc = _run(X, u, Z, 64)
    perm = np.random.RandomState(5).permutation(len(X))
    idx_p, sc_p = _run(X[perm], u[perm], Z, 64)
    assert np.array_equal(perm[idx_p], idx)
    assert np.array_equal(_bits(sc_p), _bits(sc))


def test_ties_go_to_the_lower_index(gpu):
    X = np.tile(np.arange(6, dtype=np.float32), (70, 1))
    Z = np.zeros((1, 6), np.float32)
    u = np.full(70, 0.25, np.float32)
    idx, sc = _run(X, u, Z, 70)
    assert np.array_equal(idx, np.arange(70))
    want = _emulate(X, Z, u, 70)
    assert np.array_equal(_bits(sc), _bits(want[1]))
    # two identical rows holding the top score, far apart in the pool (different workgroups): the lower index first
    X, Z, u = _integer_case(600, 9, 2, 9)
    X[[17, 555]] = 8.0
    u[[17, 555]] = 0.99
    idx, _ = _run(X, u, Z, 3)
    want_idx, _ = _emulate(X, Z, u, 3)
    assert idx[0] == 17 and 555 not in idx[:2].tolist() and np.array_equal(idx, want_idx)


def test_a_burst_of_duplicates_gets_one_pick(gpu):
    """what the rule is for: 32 copies of one row all hold the top utility; plain top-k would spend the whole batch of 16 on
    them, the ranked batch takes exactly one"""
    from a_link_amd import uncertainty as U
    N, D, M, k = 512, 16, 4, 16
    rng = np.random.RandomState(12)
    X = rng.randint(-8, 9, (N, D)).astype(np.float32)
    X[:32] = np.where(np.arange(D) % 2 == 0, 8.0, -8.0).astype(np.float32)
    Z = rng.randint(-8, 9, (M, D)).astype(np.float32)
    u = (rng.rand(N) * 0.5).astype(np.float32)
    u[:32] = 0.9
    top, _ = U.topk_device(torch.from_numpy(u).cuda(), k)
    assert (top.cpu().numpy() < 32).all()
    want_idx, want_sc = _emulate(X, Z, u, k)
    assert (want_idx < 32).sum() == 1
    idx, sc = _run(X, u, Z, k)
    assert (idx < 32).sum() == 1 and idx[idx < 32][0] == 0                  # the copy with the lowest index
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(sc), _bits(want_sc))


def test_fixed_alpha(gpu):
    from a_link_amd import uncertainty as U
    X, Z, u = _integer_case(777, 40, 5, 31)
    # alpha = 0: the utilities alone, in uncertainty.topk_device's order
    idx, sc = _run(X, u, Z, 64, alpha=0.0)
    top, vals = U.topk_device(torch.from_numpy(u).cuda(), 64)
    assert np.array_equal(idx, top.cpu().numpy()) and np.array_equal(_bits(sc), _bits(vals.cpu().numpy()))
    # alpha = 1: farthest-point order, the utilities ignored
    idx, sc = _run(X, u, Z, 64, alpha=1.0)
    want_idx, want_sc = _emulate(X, Z, u, 64, alpha=1.0)
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(sc), _bits(want_sc))
    assert np.array_equal(idx, _emulate(X, Z, np.zeros_like(u), 64, alpha=1.0)[0])
    # in between, against the emulation
    idx, sc = _run(X, u, Z, 64, alpha=0.5)
    want_idx, want_sc = _emulate(X, Z, u, 64, alpha=0.5)
    assert np.array_equal(idx, want_idx) and np.array_equal(_bits(sc), _bits(want_sc))


def test_a_nan_utility_never_wins(gpu):
    X, Z, u = _integer_case(100, 8, 2, 41)
    u[::3] = np.nan
    idx, sc = _run(X, u, Z, 100)
    good = np.flatnonzero(~np.isnan(u))
    assert sorted(idx[:len(good)].tolist()) == good.tolist() and np.isfinite(sc[:len(good)]).all()
    assert (idx[len(good):] == -1).all()                                     # nothing but NaN scores left: no pick


def _committee(D=64):
    from a_link_amd import committee, siamese
    nets = []
    for m in range(2):
        net = siamese.SiameseNetwork((D,), "b%d" % m, 0.1, seed=40 + m)
        ws = net.siamese_net.get_weights()
        ws[4] = ws[4] * np.float32(40.0)                                     # probabilities spread over (0, 1), not 0.5 +- 0.02
        net.siamese_net.set_weights(ws)
        nets.append(net)
    return committee.Bagging(nets, [])


def test_bagging_ranked_batch_indexed_and_errors(gpu):
    from a_link_amd import batch as B, uncertainty as U
    D, N, k = 64, 500, 24
    rng = np.random.RandomState(8)
    bag = _committee(D)
    L, R = torch.from_numpy(_unit(rng.randn(50, D))).cuda(), torch.from_numpy(_unit(rng.randn(9, D))).cuda()
    li = torch.from_numpy(rng.randint(0, 50, N).astype(np.int32)).cuda()
    ri = torch.from_numpy(rng.randint(0, 9, N).astype(np.int32)).cuda()
    labeled = (L[:5] - R[:5]).abs()
    mean = bag.predict_indexed(L, R, li, ri)
    for kind in ("entropy", "uncertainty"):
        got_idx, got_sc = bag.ranked_batch_indexed(L, R, li, ri, labeled, k, kind=kind)
        util = U.score_device(mean, kind)
        want_idx, want_sc = B.ranked_batch_device((L, R, li, ri), util, labeled, k)
        assert got_idx.shape == (k,) and torch.equal(got_idx, want_idx) and torch.equal(got_sc, want_sc)
        rows = (L[li.long()] - R[ri.long()]).abs()
        row_idx, row_sc = B.ranked_batch_device(rows, util, labeled, k)
        assert torch.equal(row_idx, want_idx) and torch.equal(row_sc, want_sc)
    got_idx, _ = bag.ranked_batch_indexed(L, R, li, ri, labeled, k, kind="vote_entropy", alpha=0.5)
    want_idx, _ = B.ranked_batch_device((L, R, li, ri), bag.disagreement_indexed(L, R, li, ri, kind="vote_entropy"), labeled, k, alpha=0.5)
    assert torch.equal(got_idx, want_idx)
    # refused by the Python entry
    util = U.score_device(mean, "entropy")
    with pytest.raises(ValueError, match="margin"):
        bag.ranked_batch_indexed(L, R, li, ri, labeled, k, kind="margin")
    with pytest.raises(ValueError, match="one feature space"):
        bag.ranked_batch_indexed([L, L], [R, R], li, ri, labeled, k)
    with pytest.raises(ValueError, match="at least one labelled row"):
        bag.ranked_batch_indexed(L, R, li, ri, labeled[:0], k)
    with pytest.raises(ValueError, match="CUDA"):
        B.ranked_batch_device((L.cpu(), R, li, ri), util, labeled, k)
    with pytest.raises(ValueError, match="CUDA"):
        B.ranked_batch_device((L, R, li, ri), util.cpu(), labeled, k)
    with pytest.raises(ValueError, match="float32"):
        B.ranked_batch_device((L.double(), R, li, ri), util, labeled, k)
    with pytest.raises(ValueError, match="int32"):
        B.ranked_batch_device((L, R, li.long(), ri), util, labeled, k)
    with pytest.raises(ValueError, match="D = 63"):
        B.ranked_batch_device((L, R, li, ri), util, labeled[:, :63], k)
    with pytest.raises(ValueError, match="D = 32"):
        B.ranked_batch_device((L, R[:, :32], li, ri), util, labeled, k)
    with pytest.raises(ValueError, match="outside its table"):
        B.ranked_batch_device((L, R, li, ri + 1), util, labeled, k)
    with pytest.raises(ValueError, match="utility"):
        B.ranked_batch_device((L, R, li, ri), util[:-1], labeled, k)
    with pytest.raises(ValueError, match="alpha"):
        B.ranked_batch_device((L, R, li, ri), util, labeled, k, alpha=1.5)


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    x = torch.zeros((8, 4), device="cuda")
    u = torch.zeros(8, device="cuda")
    idx = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    sc = torch.zeros(8, device="cuda")
    scratch = torch.empty(lib.alink_ranked_batch_scratch_bytes(8, 8) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(N=8, D=4, M=8, k=4, alpha=-1.0, labeled=x, scratch_ptr=sp):
        return lib.alink_ranked_batch(gpu.ptr(x), None, None, None, N, D, gpu.ptr(labeled), M, gpu.ptr(u), k, alpha, gpu.ptr(idx), gpu.ptr(sc),
                                      C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(D=0), "D=0"), (dict(D=8193), "D=8193"), (dict(M=0), "M=0"),
                     (dict(k=0), "k=0"), (dict(alpha=1.25), "alpha=1.25"), (dict(labeled=None), "NULL"), (dict(scratch_ptr=sp + 4), "aligned")):
        assert call(**kw) == -1, kw                                           # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(M=0), "alink_ranked_batch")
    torch.cuda.synchronize()
    assert bool((idx == -7).all())                                            # a refused call launches nothing
    assert call(k=100) == 0                                                   # k beyond N is clipped, not refused
    torch.cuda.synchronize()
    assert np.array_equal(idx.cpu().numpy(), np.arange(8))                    # eight identical rows: the order of the indices
