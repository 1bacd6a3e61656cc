"""GPU: k-means++ seeding on device (alink_kmeanspp, kmeanspp.hip) — bit equality with the host rule (badge.kmeans_pp) on inputs
that admit no rounding, the draw enumerated exactly, exhaustion, the pair form against the row form, real-valued rows within the
float32 accumulation bound, badge_device and Bagging.badge_indexed, what the rule is for, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_badge_host import ENUM_X, exhaustion_pool

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(rows, k, uniforms, first=None):
    from a_link_amd import badge
    dev_rows = tuple(_dev(a) for a in rows) if isinstance(rows, tuple) else _dev(rows)
    idx, pot = badge.kmeans_pp_device(dev_rows, k, uniforms=uniforms, first=first)
    assert idx.dtype == torch.int32 and pot.dtype == torch.float64 and idx.is_cuda and pot.is_cuda
    return idx.cpu().numpy(), pot.cpu().numpy()


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(got, want):
    """idx equal and potential equal bit for bit (NaN included)"""
    return np.array_equal(got[0], want[0].astype(np.int32)) and np.array_equal(_bits64(got[1]), _bits64(want[1]))


def _unit(a):
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


# (N, D, k): N off the chunk's 8 rows and the wave's two, D off 4 and off the 256-element lane sweep, D above 256 and above 512
# (second and third sweep), a pool taken whole, one row, k beyond N, and N beyond one sweep of the capped grid (2,048 chunks of
# 8 rows = 16,384: chunks of 16 rows, the last one short, and of 24)
SHAPES = [(777, 40, 64), (1031, 512, 64), (300, 7, 300), (1, 5, 1), (4, 6, 10), (130, 600, 8), (16391, 12, 8), (40000, 128, 8)]


@pytest.mark.parametrize("N,D,k", SHAPES)
def test_bit_equal_to_the_host_rule(gpu, N, D, k):
    """features in [-8, 8]: every d2 is an integer below 2^24 (exact in float32 in any order), every float64 sum an integer
    below 2^53 (exact in any order) — the device must give the host's picks and potentials bit for bit"""
    from a_link_amd import badge
    rng = np.random.RandomState(200 + N)
    X = rng.randint(-8, 9, (N, D)).astype(np.float32)
    u = rng.random_sample(k)
    for first in (None, N // 3):
        want = badge.kmeans_pp(X, k, u, first=first)
        assert want[0].shape == (min(k, N),) and (want[0] >= 0).all()      # no pool runs out: nothing is hidden behind a -1
        got = _run(X, k, u, first=first)
        assert got[0].shape == (min(k, N),)
        assert _same(got, want), (first, got[0][:8], want[0][:8])
        assert np.isnan(got[1][0])


def test_a_chunk_longer_than_one_scan_segment(gpu):
    """N = 140,001 gives chunks of 72 rows: the prologue scans the chosen chunk 64 rows at a time, so a pick in a chunk's last 8
    rows comes out of the second segment, whose sums start from the first one's total"""
    from a_link_amd import badge
    N, D, k = 140001, 4, 24
    rng = np.random.RandomState(31)
    X = rng.randint(-8, 9, (N, D)).astype(np.float32)
    u = rng.random_sample(k)
    want = badge.kmeans_pp(X, k, u)
    assert (want[0] >= 0).all() and (want[0][1:] % 72 >= 64).sum() >= 2
    assert _same(_run(X, k, u), want)


def test_the_draw_enumerated_on_the_device(gpu):
    """the 14-row pool whose weights after pick 0 sum to 64: uniforms[1] = j / 64 gives target j exactly, and the 64 second
    picks hit every row as often as its weight"""
    w = ENUM_X ** 2
    C_ = np.cumsum(w)
    hist = np.zeros(len(w), np.int64)
    X = ENUM_X[:, None].astype(np.float32)
    for j in range(64):
        idx, pot = _run(X, 2, [0.0, j / 64.0], first=0)
        assert idx[0] == 0 and pot[1] == 64.0
        assert idx[1] == np.flatnonzero(C_ > j)[0]                          # on a boundary the NEXT row with a weight
        hist[idx[1]] += 1
    assert np.array_equal(hist, w.astype(np.int64)) and hist[0] == 0 and hist[4] == 0


def test_exhaustion_and_the_all_duplicates_pool(gpu):
    from a_link_amd import badge
    X, _ = exhaustion_pool()
    u = np.random.RandomState(6).random_sample(20)
    for first in (None, 17):
        want = badge.kmeans_pp(X, 20, u, first=first)
        assert (want[0][:12] >= 0).all() and (want[0][12:] == -1).all()
        assert _same(_run(X, 20, u, first=first), want)
    same = np.tile(np.arange(6, dtype=np.float32), (70, 1))
    want = badge.kmeans_pp(same, 5, u[:5])
    assert want[0].tolist() == [0, -1, -1, -1, -1]
    assert _same(_run(same, 5, u[:5]), want)
    nan = np.full((9, 4), np.nan, np.float32)                                # no row has a norm that is a number
    want = badge.kmeans_pp(nan, 3, u[:3])
    assert want[0].tolist() == [-1, -1, -1]
    assert _same(_run(nan, 3, u[:3]), want)
    mixed = X.copy()
    mixed[5] = np.nan                                                        # a NaN row never wins, nor stops the others
    want = badge.kmeans_pp(mixed, 12, u[:12])
    assert 5 not in want[0].tolist()
    assert _same(_run(mixed, 12, u[:12]), want)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D, integer):
    """row n = |L[li[n]] - R[ri[n]]| formed on the fly == the row form on the materialised rows, bit for bit: one summation
    order for both.  D = 7 runs the scalar loads."""
    from a_link_amd import badge
    N, k = 1001, 48
    rng = np.random.RandomState(5 * D + integer)
    nl, nr = 37, 11
    if integer:                                                              # in [-4, 4]: |l - r| in [0, 8]
        L, R = rng.randint(-4, 5, (nl, D)).astype(np.float32), rng.randint(-4, 5, (nr, D)).astype(np.float32)
    else:
        L, R = _unit(rng.randn(nl, D)), _unit(rng.randn(nr, D))
    li, ri = rng.randint(0, nl, N).astype(np.int32), rng.randint(0, nr, N).astype(np.int32)
    rows = np.abs(L[li] - R[ri])
    u = rng.random_sample(k)
    got_r = _run(rows, k, u)
    got_p = _run((L, R, li, ri), k, u)
    assert _same(got_p, got_r)
    assert _same(_run((L, R, li, ri), k, u, first=7), _run(rows, k, u, first=7))
    if integer:
        assert _same(got_p, badge.kmeans_pp(rows, k, u))


def test_rows_off_the_vector_alignment(gpu):
    """a row table 4 bytes off a 16-byte boundary takes the scalar loads: same bits"""
    from a_link_amd import badge
    rng = np.random.RandomState(11)
    X = np.abs(_unit(rng.randn(300, 40)) - _unit(rng.randn(300, 40)))
    u = rng.random_sample(32)
    want = _run(X, 32, u)
    flat = torch.empty(300 * 40 + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(300, 40)
    view.copy_(torch.from_numpy(X))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    idx, pot = badge.kmeans_pp_device(view, 32, uniforms=u)
    assert _same((idx.cpu().numpy(), pot.cpu().numpy()), want)


@pytest.mark.parametrize("N,D", [(1003, 512), (1003, 40)])
def test_real_valued_picks_are_the_draws_within_the_float32_bound(gpu, N, D):
    """Follow the device's own picks with d2 and C in float64.  The device's d2 is a float32 sum of D squares of differences
    that are each rounded once: at most g = (D + 8) 2^-24 relative error (D + 2 for the sum, the rest for the float64 sums'
    own roundoff and slack), and a minimum of such values, a sum of them and a product with u carry no more.  So the device's
    pick p at step t must satisfy  w_p > 0,  C_(p-1) (1 - g) <= u T (1 + g),  u T (1 - g) <= C_p (1 + g),  and the potential
    it reports is T within g relative.  Every pick is checked.  Two runs of the same call are bit-equal."""
    k = 32
    rng = np.random.RandomState(7 + D)
    X = np.abs(_unit(rng.randn(N, D)) - _unit(rng.randn(N, D)))
    u = rng.random_sample(k)
    idx, pot = _run(X, k, u)
    again = _run(X, k, u)
    assert _same(again, (idx, pot))
    g = (D + 8) * 2.0 ** -24
    X64 = X.astype(np.float64)
    n2 = (X64 * X64).sum(axis=1)
    assert n2[idx[0]] * (1 + g) >= n2.max() * (1 - g) and np.isnan(pot[0])   # the largest norm, within the same bound
    d2 = ((X64 - X64[idx[0]]) ** 2).sum(axis=1)
    worst = 0.0
    for t in range(1, k):
        p = int(idx[t])
        assert 0 <= p < N
        w = np.where(d2 > 0, d2, 0.0)
        Cs = np.cumsum(w)
        T = Cs[-1]
        target = u[t] * T
        below = Cs[p - 1] if p > 0 else 0.0
        print("t=%d pick=%d w=%.6g C_(p-1)=%.17g uT=%.17g C_p=%.17g potential=%.17g T=%.17g" % (t, p, w[p], below, target, Cs[p], pot[t], T))
        assert w[p] > 0
        assert below * (1 - g) <= target * (1 + g)
        assert target * (1 - g) <= Cs[p] * (1 + g)
        assert abs(pot[t] - T) <= g * T
        worst = max(worst, abs(pot[t] - T) / T)
        d2 = np.minimum(d2, ((X64 - X64[p]) ** 2).sum(axis=1))
    print("D=%d: largest relative difference of the potential %.3e (g = %.3e)" % (D, worst, g))
    assert len(set(idx.tolist())) == k


def _head(D=64, seed=3):
    from a_link_amd.head import DenseHead
    hd = DenseHead(D, lr=0.1, seed=seed)
    ws = hd.get_weights()
    ws[4] = ws[4] * np.float32(40.0)                                        # probabilities spread over (0, 1), not 0.5 +- 0.02
    hd.set_weights(ws)
    return hd


def _committee(D, members=3):
    from a_link_amd import committee, siamese
    nets = []
    for m in range(members):
        net = siamese.SiameseNetwork((D,), "k%d" % m, 0.1, seed=80 + m)
        ws = net.siamese_net.get_weights()
        ws[4] = ws[4] * np.float32(40.0)
        net.siamese_net.set_weights(ws)
        nets.append(net)
    return committee.Bagging(nets, [])


def test_badge_device_and_bagging_badge_indexed(gpu):
    from a_link_amd import badge
    D, n_pairs, k = 64, 300, 16
    rng = np.random.RandomState(9)
    L, R = _dev(_unit(rng.randn(40, D))), _dev(_unit(rng.randn(9, D)))
    li, ri = _dev(rng.randint(0, 40, n_pairs).astype(np.int32)), _dev(rng.randint(0, 9, n_pairs).astype(np.int32))
    u = rng.random_sample(k)
    hd = _head(D)
    emb = hd.expected_gradient_length_device(L, R, li, ri, want=("emb",))["emb"]
    assert emb.shape == (n_pairs, 128)
    want = badge.kmeans_pp_device(emb, k, uniforms=u)
    for got in (badge.badge_device(hd, L, R, li, ri, n_instances=k, uniforms=u), hd.badge_device(L, R, li, ri, n_instances=k, uniforms=u)):
        assert torch.equal(got[0], want[0]) and np.array_equal(_bits64(got[1].cpu().numpy()), _bits64(want[1].cpu().numpy()))
    a, b = hd.badge_device(L, R, li, ri, n_instances=k, seed=4), hd.badge_device(L, R, li, ri, n_instances=k, seed=4)
    assert torch.equal(a[0], b[0]) and a[0].numel() == k
    plain = hd.badge_device(L[:9].contiguous(), R, n_instances=4, uniforms=u)             # without li / ri: pair n is (L[n], R[n])
    assert torch.equal(plain[0], badge.kmeans_pp_device(hd.expected_gradient_length_device(L[:9].contiguous(), R, want=("emb",))["emb"], 4, uniforms=u)[0])
    bag = _committee(D)
    embs = [m.siamese_net.expected_gradient_length_device(L, R, li, ri, want=("emb",))["emb"] for m in bag.models]
    want = badge.kmeans_pp_device(torch.cat(embs, dim=1), k, uniforms=u)
    for got in (bag.badge_indexed(L, R, li, ri, k, uniforms=u), bag.badge_indexed([L] * 3, [R] * 3, li, ri, k, uniforms=u)):
        assert torch.equal(got[0], want[0]) and np.array_equal(_bits64(got[1].cpu().numpy()), _bits64(want[1].cpu().numpy()))
    idx, inst = badge.badge_sampling(hd, [L[:9].contiguous(), R], n_instances=4, random_state=2)   # the sampler's device route
    assert idx.shape == (4,) and torch.equal(inst[0], L[torch.from_numpy(idx).cuda()]) and torch.equal(inst[1], inst[0])
    assert np.array_equal(idx, hd.badge_device(L[:9].contiguous(), R, n_instances=4, seed=2)[0].cpu().numpy())


def test_a_burst_of_duplicates_gets_one_pick_each(gpu):
    """what it is for: 40 distinct pairs, each ten times in the pool.  A BADGE batch of 40 never takes a pair twice (a duplicate
    of a centre has d2 = 0 exactly and no weight); the plain top-40 by expected gradient length spends its batch on the ten
    copies of a few pairs"""
    D, k = 64, 40
    rng = np.random.RandomState(13)
    L, R = _dev(_unit(rng.randn(40, D))), _dev(_unit(rng.randn(40, D)))
    li = np.repeat(np.arange(40, dtype=np.int32), 10)
    perm = rng.permutation(400)
    li, ri = li[perm], li[perm].copy()
    hd = _head(D)
    idx, pot = hd.badge_device(L, R, _dev(li), _dev(ri), n_instances=k, seed=1)
    idx = idx.cpu().numpy()
    taken = [(li[i], ri[i]) for i in idx if i >= 0]
    assert len(taken) == len(set(taken)) and len(taken) >= 2
    egl_ = hd.expected_gradient_length_device(L, R, _dev(li), _dev(ri))["egl"]
    top = torch.topk(egl_, k).indices.cpu().numpy()
    assert len({(li[i], ri[i]) for i in top}) < len(set(taken))


def test_python_refusals(gpu):
    from a_link_amd import badge
    rng = np.random.RandomState(3)
    X = _dev(rng.randn(50, 8).astype(np.float32))
    u = rng.random_sample(5)
    run = badge.kmeans_pp_device
    with pytest.raises(ValueError, match="CUDA"):
        run(X.cpu(), 5, uniforms=u)
    with pytest.raises(ValueError, match="float32"):
        run(X.double(), 5, uniforms=u)
    with pytest.raises(ValueError, match="uniforms"):
        run(X, 5, uniforms=u[:4])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        run(X, 5, uniforms=[0.0, 0.5, 1.0, 0.5, 0.5])
    with pytest.raises(ValueError, match=r"\[0, 1\)"):
        run(X, 5, uniforms=[0.0, 0.5, -0.25, 0.5, 0.5])
    with pytest.raises(ValueError, match="first"):
        run(X, 5, uniforms=u, first=50)
    with pytest.raises(ValueError, match="n_instances"):
        run(X, 0, uniforms=u)
    li = _dev(np.arange(4, dtype=np.int32))
    with pytest.raises(ValueError, match="int32"):
        run((X, X, li.long(), li), 2, uniforms=u)
    with pytest.raises(ValueError, match="outside its table"):
        run((X, X, li + 47, li), 2, uniforms=u)
    # the committee's embedding side by side: 65 members x 2 x 64 = 8,320 columns, beyond the 8,192 a picked row may have
    bag = _committee(64, members=1)
    from a_link_amd import committee
    wide = committee.Bagging(bag.models * 65, [])
    L = _dev(_unit(rng.randn(6, 64)))
    with pytest.raises(ValueError, match="D = 8320"):
        wide.badge_indexed(L, L, li, li, 2)
    with pytest.raises(ValueError, match="feature matrices"):
        bag.badge_indexed([L, L], [L, L], li, li, 2)

    class Host(object):
        siamese_net = None
    with pytest.raises(TypeError, match="DenseHead"):
        committee.Bagging([Host()], []).badge_indexed(L, L, li, li, 2)
    with pytest.raises(TypeError):
        badge.badge_sampling(object(), [L, L])


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    x = torch.zeros((8, 4), device="cuda")
    ind = torch.zeros(8, dtype=torch.int32, device="cuda")
    u = torch.full((8,), 0.5, dtype=torch.float64, device="cuda")
    idx = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    pot = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    scratch = torch.empty(lib.alink_kmeanspp_scratch_bytes(8, 8) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(x_=x, r=None, li=None, ri=None, N=8, D=4, u_=u, first=-1, k=4, idx_=idx, pot_=pot, scratch_ptr=sp):
        return lib.alink_kmeanspp(gpu.ptr(x_), gpu.ptr(r), gpu.ptr(li), gpu.ptr(ri), N, D, gpu.ptr(u_), first, k, gpu.ptr(idx_), gpu.ptr(pot_),
                                  C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(x_=None), "NULL"), (dict(u_=None), "NULL"), (dict(idx_=None), "NULL"), (dict(pot_=None), "NULL"),
                     (dict(scratch_ptr=0), "NULL"), (dict(li=ind), "pair form"), (dict(li=ind, r=x), "pair form"), (dict(li=ind, ri=ind), "pair form"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(D=0), "D=0"), (dict(D=8193), "D=8193"),
                     (dict(k=0), "k=0"), (dict(k=-3), "k=-3"), (dict(first=-2), "first=-2"), (dict(first=8), "first=8"),
                     (dict(scratch_ptr=sp + 4), "aligned")):
        assert call(**kw) == -1, kw                                           # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(k=0), "alink_kmeanspp")
    torch.cuda.synchronize()
    assert bool((idx == -7).all()) and bool((pot == -7.0).all())              # a refused call launches nothing
    assert call(k=100) == 0                                                   # k beyond N is clipped, not refused
    torch.cuda.synchronize()
    assert idx.cpu().tolist() == [0] + [-1] * 7                               # eight identical rows: one centre, then nothing to draw
    assert np.isnan(pot[0].item()) and bool((pot[1:] == 0).all())
