"""GPU: facility-location gains, cover and greedy selection on device (alink_facility_gains, alink_facility_cover,
alink_facility_select, facility.hip; a-link_amd/facility.py) — bit equality with the host rule on small-integer rows with an integer
cur around every size the kernels have, the score shared with ProbCover bit for bit, the pair form against the row form, real-valued
gains within the float32 band of a D-term chain summed over the pool, real-valued picks step by step, rows that are not finite,
every refusal, and the end-to-end forms."""
import numpy as np
import pytest
import torch

from test_gpu_knn import _pair_of
from test_typiclust_host import int_rows

pytestmark = pytest.mark.gpu

FLT_MAX = float(np.finfo(np.float32).max)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _np(t):
    return t.cpu().numpy()


def _int_cur(N, seed, hi=200):
    return np.random.RandomState(300 + N + seed).randint(0, hi, N).astype(np.float32)


# ---- 1. gains, bit for bit ---------------------------------------------------------------------------------------------------
# (N, R, D): a lone row; below / on / above a 32-block and a 128-tile of candidates and of pool rows; D tails and D = 1; 16-byte
# loads (D % 4 == 0) and scalar ones; (300, 5, 7) and (1000, 130, 64): several slabs with a partial last one
GAIN_SHAPES = [(1, 1, 1), (33, 5, 33), (127, 127, 3), (128, 128, 32), (129, 1, 130), (257, 129, 33), (300, 5, 7), (1000, 130, 64)]


@pytest.mark.parametrize("N,R,D", GAIN_SHAPES)
def test_gains_equal_the_host_bit_for_bit(gpu, N, R, D):
    from a_link_amd import facility
    X, cur = int_rows(N, D), _int_cur(N, D)
    cand = np.random.RandomState(N + R).randint(0, N, R).astype(np.int32)
    got = facility.gains_device(_dev(X), _dev(cur), cand)
    assert got.dtype == torch.float64 and got.shape == (R,)
    assert _same(_np(got), facility.gains(X, cur, cand))
    assert _same(_np(facility.gains_device(_dev(X), _dev(cur), _dev(cand))), _np(got))             # two runs of a call agree
    perm = np.random.RandomState(R).permutation(R)
    assert _same(_np(facility.gains_device(_dev(X), _dev(cur), cand[perm])), _np(got)[perm])       # the list permuted


def test_gains_of_every_row_and_of_a_list_with_strays(gpu):
    from a_link_amd import facility
    N, D = 300, 32
    X, cur = int_rows(N, D), _int_cur(N, 1, hi=400)
    got = _np(facility.gains_device(_dev(X), _dev(cur)))                                           # cand NULL: position r = row r
    assert _same(got, facility.gains(X, cur))
    assert _same(_np(facility.gains_device(_dev(X), _dev(cur), np.arange(N))), got)
    cand = np.array([7, 7, -1, N, 299, 0, 7, -5, N + 1000, 128, 127, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)
    stray = _np(facility.gains_device(_dev(X), _dev(cur), cand))
    assert _same(stray, facility.gains(X, cur, cand))
    assert stray[0] == stray[1] == stray[6] == got[7] and stray[2] == stray[3] == stray[7] == stray[8] == stray[11] == stray[12] == 0


# ---- 2. cover, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1, 33, 128, 129, 300])
def test_cover_equals_the_host_bit_for_bit(gpu, S):
    from a_link_amd import facility
    N, D = 257, 33
    X, cur = int_rows(N, D, seed=S), _int_cur(N, S, hi=600)
    sel = np.random.RandomState(S).randint(-1, N + 2, S).astype(np.int32)                          # -1 and out-of-range among them
    if S:
        sel[0] = 5
    before = _dev(cur)
    got = facility.cover_device(_dev(X), before, sel)
    assert _same(_np(got), facility.cover(X, cur, sel)) and _same(_np(before), cur)
    if S == 0:
        assert _same(_np(got), cur)
    if S == 1:
        assert _same(_np(facility.cover_device(_dev(X), before, np.array([-1], np.int32))), cur)   # a lone stray: nothing changes


def test_cover_forms_the_score_of_the_ball_graph(gpu):
    """covering group 0 from FLT_MAX with group 1's rows is max(t_other, 0) of ProbCover's purity pass, bit for bit: one formula"""
    from a_link_amd import facility, probcover
    N, D = 300, 33
    X = np.random.RandomState(N + D).randn(N, D).astype(np.float32)
    X[10] = X[200]                                                                                 # a coinciding pair across the groups
    groups = (np.arange(N) >= 150).astype(np.int32)
    t_other, _ = probcover.nearest_other_device(_dev(X), _dev(groups))
    cur = facility.cover_device(_dev(X), torch.full((N,), FLT_MAX, device="cuda"), np.flatnonzero(groups == 1))
    want = np.maximum(_np(t_other), np.float32(0))
    assert _same(_np(cur)[:150], want[:150]) and (_np(cur)[:150] < FLT_MAX).all()


# ---- 3. select, bit for bit --------------------------------------------------------------------------------------------------
def _select_both(X, cur, k, cand):
    from a_link_amd import facility
    got = tuple(_np(t) for t in facility.select_device(_dev(X), _dev(cur), k, cand))
    want = facility.select(X, cur, k, cand)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.float32
    assert all(_same(g, w) for g, w in zip(got, want)), (got[0], want[0])
    return got


@pytest.mark.parametrize("N,D,k,R", [(300, 33, 12, None), (600, 7, 16, 96), (129, 130, 8, 129)])
def test_select_equals_the_host_bit_for_bit(gpu, N, D, k, R):
    from a_link_amd import facility
    X = int_rows(N, D)
    cur = np.full(N, facility.default_cap(X), np.float32)
    cand = None if R is None else np.random.RandomState(N + k).randint(0, N, (k, R)).astype(np.int32)
    picks, gain, _ = _select_both(X, cur, k, cand)
    assert (picks >= 0).all() and len(set(picks.tolist())) == k and (gain > 0).all()


def test_select_on_identical_rows_and_chained(gpu):
    from a_link_amd import facility
    X = np.tile(int_rows(1, 9), (140, 1))
    picks, gain, cur = _select_both(X, np.full(140, 50.0, np.float32), 3, None)
    assert picks.tolist() == [0, -1, -1] and gain.tolist() == [7000.0, 0.0, 0.0] and (cur == 0).all()
    picks, _, _ = _select_both(X, np.full(140, 50.0, np.float32), 2, np.array([[139, 4, 139], [4, 4, 4]], np.int32))
    assert picks.tolist() == [139, -1]                                                            # the lower POSITION wins
    # real-valued rows: one select = chained gains + argmax + cover, and k1 + k2 chained selects = one call
    N, D, k = 300, 40, 6
    Y = _dev(np.random.RandomState(5).randn(N, D).astype(np.float32))
    cur0 = torch.full((N,), float(facility.default_cap(_np(Y))), device="cuda")
    cand = np.random.RandomState(6).randint(0, N, (k, 50)).astype(np.int32)
    for c in (None, cand):
        picks, gain, cur = facility.select_device(Y, cur0, k, c)
        step = cur0
        for t in range(k):
            g = facility.gains_device(Y, step, None if c is None else c[t])
            pos = int(torch.argmax(g))                                                             # the first of equal maxima
            assert float(g[pos]) > 0 and int(picks[t]) == (pos if c is None else int(c[t][pos])) and _same(_np(gain[t]), _np(g[pos]))
            step = facility.cover_device(Y, step, picks[t:t + 1])
        assert _same(_np(step), _np(cur))
        p1, g1, c1 = facility.select_device(Y, cur0, 2, None if c is None else c[:2])
        p2, g2, c2 = facility.select_device(Y, c1, 4, None if c is None else c[2:])
        assert _same(_np(torch.cat([p1, p2])), _np(picks)) and _same(_np(torch.cat([g1, g2])), _np(gain)) and _same(_np(c2), _np(cur))


# ---- 4. the pair form ----------------------------------------------------------------------------------------------------------
def _all_three(rows, cur, cand, sel, k):
    from a_link_amd import facility
    out = [facility.gains_device(rows, cur, cand[0]), facility.cover_device(rows, cur, sel)]
    out += list(facility.select_device(rows, cur, k, cand))
    return [_np(t) for t in out]


@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_the_row_form(gpu, D):
    rng = np.random.RandomState(D)
    N, P, G, k = 200, 37, 23, 4
    L, R = rng.randn(P, D).astype(np.float32), rng.randn(G, D).astype(np.float32)
    li, ri = rng.randint(0, P, N).astype(np.int32), rng.randint(0, G, N).astype(np.int32)
    Q = np.abs(L[li] - R[ri])                                                                      # one rounded subtraction: the on-the-fly row's bits
    cur = _dev(np.full(N, 4 * (Q.astype(np.float64) ** 2).sum(axis=1).max(), np.float32))
    cand, sel = rng.randint(0, N, (k, 60)).astype(np.int32), rng.randint(0, N, 9).astype(np.int32)
    want = _all_three(_dev(Q), cur, cand, sel, k)
    got = _all_three((_dev(L), _dev(R), _dev(li), _dev(ri)), cur, cand, sel, k)
    assert all(_same(g, w) for g, w in zip(got, want))

    def off(a):                                                                                    # 4 bytes off the 16-byte alignment: the scalar loads
        buf = torch.empty(a.size + 1, device="cuda")
        buf[1:] = _dev(a).reshape(-1)
        t = buf[1:].view(a.shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    assert all(_same(g, w) for g, w in zip(_all_three(off(Q), cur, cand, sel, k), want))
    assert all(_same(g, w) for g, w in zip(_all_three((off(L), _dev(R), _dev(li), _dev(ri)), cur, cand, sel, k), want))
    assert all(_same(g, w) for g, w in zip(_all_three((_dev(L), off(R), _dev(li), _dev(ri)), cur, cand, sel, k), want))


# ---- 5. real-valued gains ------------------------------------------------------------------------------------------------------
def _tol(X, gain_host, cand):
    """tol(c) = sum_n (D + 9) 2^-24 (|x_n| + |x_c|)^2 + 2^-24 gain(c): ProbCover's per-score band summed over the pool, plus the
    term's one subtraction"""
    X = np.asarray(X, np.float64)
    nrm = np.sqrt((X * X).sum(axis=1))
    D = X.shape[1]
    return np.array([((D + 9) * 2.0 ** -24 * (nrm + nrm[c]) ** 2).sum() for c in cand]) + 2.0 ** -24 * gain_host


@pytest.mark.parametrize("N,D", [(600, 33), (1000, 64), (300, 130)])
def test_real_valued_gains_lie_within_the_float32_band(gpu, N, D):
    """The worst |device - host| / tol over all candidates is printed.  Seen on one MI355X: 0.0051, 0.0036 and 0.0018 at the three
    shapes; a float32 NumPy emulation of the rule reaches at most 1.7 % of tol at these shapes."""
    from a_link_amd import facility
    X = np.random.RandomState(N + D).randn(N, D).astype(np.float32)
    cur = facility.cover(X, np.full(N, facility.default_cap(X), np.float32), [0, N // 2])          # a float32 cur, shared
    got = _np(facility.gains_device(_dev(X), _dev(cur)))
    want = facility.gains(X, cur)
    ratio = np.abs(got - want) / _tol(X, want, np.arange(N))
    print("facility gains (%d, %d): worst |device - host| / tol = %.4f" % (N, D, ratio.max()))
    assert (ratio <= 1.0).all(), ratio.max()                                                       # no candidate is exempt


# ---- 6. real-valued picks, step by step --------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [None, 96])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_real_valued_picks_step_by_step(gpu, R, seed):
    """The host continues from the device's cur; a device pick that differs from the host's is accepted only if the host's gains of
    the two differ by at most tol(a) + tol(b), and at most one step in eight may be so exempt.  Seen on one MI355X: 0 exempt
    steps in all six cases."""
    from a_link_amd import facility
    N, D, k = 600, 33, 16
    X = np.random.RandomState(seed).randn(N, D).astype(np.float32)
    Xd = _dev(X)
    cur = torch.full((N,), float(facility.default_cap(X)), device="cuda")
    cand = None if R is None else np.random.RandomState(100 + seed).randint(0, N, (k, R)).astype(np.int32)
    exempt = 0
    for t in range(k):
        ct = np.arange(N) if cand is None else cand[t]
        g = facility.gains(X, _np(cur), ct)
        pos = int(np.argmax(g))
        picks, _, cur = facility.select_device(Xd, cur, 1, None if cand is None else cand[t:t + 1])
        p = int(picks[0])
        assert p >= 0 and p in ct
        if p != ct[pos]:
            other = int(np.flatnonzero(ct == p)[0])
            tol = _tol(X, g[[pos, other]], ct[[pos, other]])
            assert abs(g[pos] - g[other]) <= tol.sum(), (t, p, ct[pos], g[pos], g[other], tol)
            exempt += 1
    print("facility picks (R=%s, seed %d): %d of %d steps exempt" % (R, seed, exempt, k))
    assert exempt <= k // 8


# ---- 7. rows and cur entries that are not finite ------------------------------------------------------------------------------
def test_non_finite_rows_and_cur(gpu):
    from a_link_amd import facility
    N, D = 200, 12
    X, cur = int_rows(N, D, seed=4), _int_cur(N, 4, hi=300)
    X[17, 3] = np.nan
    X[140, 0] = np.inf
    X[141, 5] = -np.inf
    cur[60] = np.nan
    bad = [17, 140, 141]
    got = _np(facility.gains_device(_dev(X), _dev(cur)))
    assert _same(got, facility.gains(X, cur)) and (got[bad] == 0).all() and np.isfinite(got).all()
    keep = np.delete(np.arange(N), bad + [60])                                                     # the bad rows and the NaN cur contribute 0:
    assert _same(got[keep], facility.gains(X[keep], cur[keep]))                                    # the gains of the pool without them
    after = facility.cover_device(_dev(X), _dev(cur), np.array([17, 140, 3, 141], np.int32))
    assert _same(_np(after), facility.cover(X, cur, [17, 140, 3, 141]))
    assert _same(_np(after)[bad + [60]], cur[bad + [60]])                                          # they keep their cur; the NaN stays
    picks, gain, end = (_np(t) for t in facility.select_device(_dev(X), _dev(cur), 10))
    want = facility.select(X, cur, 10)
    assert _same(picks, want[0]) and _same(gain, want[1]) and _same(end, want[2])
    assert not set(picks.tolist()) & set(bad) and _same(end[bad + [60]], cur[bad + [60]])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(gpu):
    from a_link_amd import net_host
    lib = gpu.init(0)
    N, D, R, k = 50, 8, 10, 3
    x = _dev(int_rows(N, D))
    ind = torch.zeros(N, dtype=torch.int32, device="cuda")
    cand = torch.zeros(k * R, dtype=torch.int32, device="cuda")
    outs = {"cur": torch.full((N,), -7.0, device="cuda"), "gain": torch.full((max(R, k),), -7.0, dtype=torch.float64, device="cuda"),
            "picks": torch.full((k,), -7, dtype=torch.int32, device="cuda")}
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_facility_scratch_bytes(N, D, N, k), x.device)
    st = gpu.current_stream(x.device)
    base = dict(x=x, r=None, li=None, ri=None, N=N, D=D, cur=outs["cur"], cand=cand, R=R, k=k, gain=outs["gain"], picks=outs["picks"],
                sel=ind, S=4, scratch=sp)

    def gains(**kw):
        a = dict(base, **kw)
        return lib.alink_facility_gains(gpu.ptr(a["x"]), gpu.ptr(a["r"]), gpu.ptr(a["li"]), gpu.ptr(a["ri"]), a["N"], a["D"], gpu.ptr(a["cur"]),
                                        gpu.ptr(a["cand"]), a["R"], gpu.ptr(a["gain"]), a["scratch"], st)

    def cover(**kw):
        a = dict(base, **kw)
        return lib.alink_facility_cover(gpu.ptr(a["x"]), gpu.ptr(a["r"]), gpu.ptr(a["li"]), gpu.ptr(a["ri"]), a["N"], a["D"], gpu.ptr(a["cur"]),
                                        gpu.ptr(a["sel"]), a["S"], a["scratch"], st)

    def select(**kw):
        a = dict(base, **kw)
        return lib.alink_facility_select(gpu.ptr(a["x"]), gpu.ptr(a["r"]), gpu.ptr(a["li"]), gpu.ptr(a["ri"]), a["N"], a["D"], gpu.ptr(a["cur"]),
                                         gpu.ptr(a["cand"]), a["R"], a["k"], gpu.ptr(a["picks"]), gpu.ptr(a["gain"]), a["scratch"], st)
    pool = [(dict(x=None), "NULL"), (dict(cur=None), "NULL"), (dict(scratch=None), "NULL"), (dict(li=ind), "pair form"),
            (dict(li=ind, r=x), "pair form"), (dict(N=0), "N="), (dict(N=2 ** 31), "N="), (dict(D=0), "D="), (dict(D=8193), "D="),
            (dict(scratch=sp + 128), "256-byte")]
    cands = [(dict(R=0), "R="), (dict(R=N + 1), "R="), (dict(cand=None), "must equal N")]
    cases = [(gains, pool + cands + [(dict(gain=None), "NULL")]),
             (cover, pool + [(dict(S=-1), "S="), (dict(sel=None), "without dev_sel")]),
             (select, pool + cands + [(dict(k=0), "k="), (dict(picks=None), "NULL"), (dict(gain=None), "NULL")])]
    for call, table in cases:
        for kw, text in table:
            assert call(**kw) == -1, (call.__name__, kw)                   # ALINK_EINVAL
            assert text in lib.alink_last_error().decode(), (call.__name__, kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(select(k=-2), "alink_facility_select")
    assert cover(S=0, sel=None) == 0                                       # a no-op, not a refusal
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs.values())               # a refused call launches nothing
    assert lib.alink_facility_scratch_bytes(N, D, N, k) >= lib.alink_facility_scratch_bytes(N, D, 1, 1) > 0
    assert gains(cand=None, R=N, gain=torch.empty(N, dtype=torch.float64, device="cuda")) == 0
    torch.cuda.synchronize()


# ---- 9. end to end ----------------------------------------------------------------------------------------------------------------
def test_facility_device_equals_the_host(gpu):
    from a_link_amd import facility
    X = int_rows(400, 24, seed=8)
    lab = np.array([5, 77, 399, 128])
    for labelled in (None, lab):
        for kw in (dict(), dict(eps=0.1, random_state=3), dict(cap=500.0)):
            want, winfo = facility.facility(X, labelled, 14, **kw)
            got, ginfo = facility.facility_device(_dev(X), labelled, 14, **kw)
            assert np.array_equal(got, want) and len(got) == 14 and got.dtype == np.int64
            assert _same(ginfo["gain"], winfo["gain"]) and ginfo["cap"] == winfo["cap"] and ginfo["objective"] == winfo["objective"]
            assert labelled is None or not set(got.tolist()) & set(lab.tolist())
    Y = np.repeat(int_rows(5, 6, seed=2), 8, axis=0)                       # five distinct rows: the fill completes the batch
    want, winfo = facility.facility(Y, [0], 9, fill="random", random_state=4)
    got, ginfo = facility.facility_device(_dev(Y), [0], 9, fill="random", random_state=4)
    assert np.array_equal(got, want) and len(got) == 9 and ginfo["exhausted"] and winfo["exhausted"]
    with pytest.raises(ValueError, match="CUDA"):
        facility.gains_device(torch.zeros(4, 3), torch.zeros(4))
    with pytest.raises(ValueError, match="cur"):
        facility.gains_device(_dev(X), torch.zeros(3, device="cuda"))
    with pytest.raises(ValueError, match="cand"):
        facility.select_device(_dev(X), torch.zeros(400, device="cuda"), 2, np.zeros((3, 5), np.int32))


class _Clf(object):
    def __init__(self, proba):
        self.proba = proba

    def predict_proba(self, X):
        return self.proba


def _committee(D, members=3):
    from a_link_amd import committee, siamese
    return committee.Bagging([siamese.SiameseNetwork((D,), "c%d" % m, 0.1, seed=80 + m) for m in range(members)], [])


def test_bagging_and_sampler_forms(gpu):
    from a_link_amd import existing_al, facility
    X = np.abs(int_rows(300, 64, seed=6))
    Lh, Rh, lih, rih = _pair_of(X)
    L, R, li, ri = (_dev(a) for a in (Lh, Rh, lih, rih))
    lab = np.array([3, 50, 299])
    bag = _committee(64)
    got, _ = bag.facility_indexed(L, R, li, ri, lab, 10, eps=0.05, random_state=1)                 # kind=None: the members are not consulted
    want, _ = facility.facility_device((L, R, li, ri), lab, 10, eps=0.05, random_state=1)
    host, _ = facility.facility(X, lab, 10, eps=0.05, random_state=1)
    assert np.array_equal(got, want) and np.array_equal(got, host) and len(got) == 10 and not set(got.tolist()) & set(lab.tolist())
    got, info = bag.facility_indexed(L, R, li, ri, lab, 6, kind="entropy", beta=5, eps=None)       # FASS over the committee's entropy
    kept = info["kept"].cpu().numpy()
    assert len(got) == 6 and len(set(got.tolist())) == 6 and not set(got.tolist()) & set(lab.tolist())
    assert len(kept) == 33 and set(got.tolist()) <= set(kept[:30].tolist()) and kept[30:].tolist() == lab.tolist()
    with pytest.raises(ValueError, match="one feature space"):
        bag.facility_indexed([L] * 3, [R] * 3, li, ri, lab, 5)
    # the sampler's device route equals its host route, on rows and on pair input
    assert existing_al.get_strategy_object("facility_sampling") is facility.facility_sampling
    rng = np.random.RandomState(9)
    p = rng.uniform(0.5, 1.0, 300)
    clf = _Clf(np.stack([p, 1 - p], axis=1))
    A, B = Lh[lih], Rh[rih]
    for kw in (dict(beta=4), dict(beta=None), dict(beta=3, eps=0.2, random_state=5)):
        want, _ = facility.facility_sampling(clf, [A, B], n_instances=8, **kw)
        idx, inst = facility.facility_sampling(clf, [_dev(A), _dev(B)], n_instances=8, **kw)
        assert np.array_equal(idx, want) and len(idx) == 8
        assert torch.equal(inst[0], _dev(A)[torch.from_numpy(idx).cuda()]) and torch.equal(inst[1], inst[0])
        idx, inst = facility.facility_sampling(clf, _dev(X), n_instances=8, **kw)
        assert np.array_equal(idx, want) and torch.equal(inst, _dev(X)[torch.from_numpy(idx).cuda()])
