"""GPU: k nearest neighbours, typicality and the per-group argmax on device (alink_knn, alink_group_argmax, knn.hip;
a-link_amd/typiclust.py) — bit equality with the host rule (typiclust.knn) on small-integer rows around every size the kernel
has, a pool where everything ties, the pair form against the row form, groups, real-valued rows within the float32 bound of a
D-term chain, non-finite rows, the TypiClust selection against the host, its Bagging form, and every refusal."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_typiclust_host import K_REAL, blobs, int_rows, random_groups, real_cases, same_lists, within_float32_bound

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rows_dev(rows):
    return tuple(_dev(a) for a in rows) if isinstance(rows, tuple) else _dev(rows)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _run(rows, k, groups=None, squared=False, eps=1e-5):
    """alink_knn with every output -> (idx, d2, found, typicality) as NumPy arrays"""
    from a_link_amd import typiclust
    out = typiclust._knn_call(_rows_dev(rows), k, None if groups is None else _dev(np.asarray(groups, np.int32)), squared, eps, True)
    idx, d2, found, typ = out
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and found.dtype == torch.int32 and typ.dtype == torch.float32
    assert idx.shape == d2.shape and idx.shape[1] == k and found.shape == typ.shape == (idx.shape[0],)
    return tuple(t.cpu().numpy() for t in out)


def _same_bits(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _check_against_host(X, k, groups, got):
    from a_link_amd import typiclust
    want = typiclust.knn(X, k, groups)
    assert same_lists(got[:3], want) is None, same_lists(got[:3], want)
    assert np.array_equal(np.isnan(got[1]), got[0] < 0)                    # unfilled slots: -1 and NaN
    typ = typiclust.typicality(X, k, groups).astype(np.float64)
    assert (np.abs(got[3] - typ) <= 2.0 ** -23 * typ).all() and (got[3][want[2] == 0] == 0).all()


# (N, D, K).  The kernel's sizes: 128 rows a workgroup (32 a wave), 128 candidates a tile in blocks of 32, 32 columns a chunk; lists of
# 8, 16 and 32; 16-byte loads where D is a multiple of 4.  Between them: a lone row, K >= N, one below / on / one above a block and
# a tile, more than one workgroup and tile, D tails, D = 1, each list size with K below and on it.
INT_SHAPES = [(1, 1, 1), (1, 33, 20), (2, 3, 5), (2, 130, 1), (33, 32, 32), (33, 33, 5), (33, 1, 20), (127, 3, 20), (127, 130, 32),
              (128, 32, 20), (128, 1, 32), (129, 33, 32), (129, 130, 1), (257, 130, 20), (257, 1, 5), (300, 3, 32), (300, 32, 5),
              (300, 33, 20)]


@pytest.mark.parametrize("N,D,K", INT_SHAPES)
def test_integer_rows_bit_equal_to_the_host_rule(gpu, N, D, K):
    """rows in -4 .. 4: every product, score and d2 is an integer far below 2^24 — exact in any order, so idx, d2 and found must
    equal the host's bit for bit, ties (there are many) included; typicality within one float32 rounding of the float64 value"""
    from a_link_amd import typiclust
    X = int_rows(N, D)
    got = _run(X, K)
    _check_against_host(X, K, None, got)
    sq = _run(X, K, squared=True, eps=0.25)
    assert _same_bits(sq[:3], got[:3])
    want = typiclust.typicality(X, K, squared=True, eps=0.25).astype(np.float64)
    assert (np.abs(sq[3] - want) <= 2.0 ** -23 * want).all()
    assert _same_bits(_run(X, K), got)                                     # two runs of a call


def test_a_pool_of_identical_rows(gpu):
    """everything ties at distance 0: the lists are the lowest indices with self left out"""
    for N, D, K in ((300, 7, 20), (129, 32, 32), (20, 3, 32)):
        X = np.tile(int_rows(1, D), (N, 1))
        idx, d2, found, typ = _run(X, K)
        for n in (0, 1, K - 1, K, K + 1, N - 1):
            if n < N:
                want = [j for j in range(N) if j != n][:K]
                assert idx[n, :len(want)].tolist() == want and (idx[n, len(want):] == -1).all()
        assert (found == min(K, N - 1)).all() and (d2[idx >= 0] == 0).all()
        assert (typ == np.float32(1.0 / 1e-5)).all()


@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D):
    rng = np.random.RandomState(D)
    P, G, N, K = 60, 9, 300, 20
    li, ri = rng.randint(0, P, N).astype(np.int32), rng.randint(0, G, N).astype(np.int32)
    groups = random_groups(N, 3)
    for integer in (True, False):
        L = rng.randint(-2, 3, (P, D)).astype(np.float32) if integer else rng.randn(P, D).astype(np.float32)
        R = rng.randint(-2, 3, (G, D)).astype(np.float32) if integer else rng.randn(G, D).astype(np.float32)
        X = np.abs(L[li] - R[ri])                           # one rounded subtraction: the bits the on-the-fly row holds
        for g in (None, groups):
            pair, row = _run((L, R, li, ri), K, g), _run(X, K, g)
            assert _same_bits(pair, row), (integer, g is None)
            if integer:
                _check_against_host(X, K, g, pair)
    # the same table 4 bytes off the 16-byte alignment (the scalar loads)
    X = rng.randn(N, D).astype(np.float32)
    buf = torch.empty(N * D + 1, device="cuda")
    buf[1:] = _dev(X).reshape(-1)
    xo = buf[1:].view(N, D)
    assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
    from a_link_amd import typiclust
    off = tuple(t.cpu().numpy() for t in typiclust._knn_call(xo, K, None, False, 1e-5, True))
    assert _same_bits(off, _run(X, K))


@pytest.mark.parametrize("G", [1, 3, 40])
def test_groups_bit_equal_to_the_host_rule(gpu, G):
    """a random labelling with rows of group -1 and -3 among it; with 40 groups most groups are smaller than K"""
    for N, D, K in ((300, 3, 20), (257, 33, 5), (129, 32, 32)):
        X = int_rows(N, D, seed=G)
        g = random_groups(N, G)
        assert (g < 0).any()
        got = _run(X, K, g)
        _check_against_host(X, K, g, got)
        assert (got[2][g < 0] == 0).all() and not np.isin(got[0], np.flatnonzero(g < 0)).any()
        if G == 40:
            assert (got[2] < K).any()
        if G == 1:
            assert ((got[0] >= 0).sum(axis=1) == got[2]).all()
    X = int_rows(300, 5)
    assert _same_bits(_run(X, 20, None), _run(X, 20, np.zeros(300, np.int32)))


def test_real_valued_rows_within_the_float32_bound(gpu):
    """test_typiclust_host.within_float32_bound on 300 x 128 rows in 3 groups and on 260 x 512 rows, K = 20: every reported
    neighbour j and every candidate i left out satisfy s(n, j) <= s(n, i) + E(n, j) + E(n, i), and so do consecutive entries.
    Measured on one MI355X: no row's set differs from the float64 set in either case; the largest excess is -0.0381 / -0.0115
    of its bound — negative: even the closest pair of scores stands in its float64 order."""
    for name, X, g in real_cases():
        idx, d2, found, typ = _run(X, K_REAL, g)
        fails, differ, worst = within_float32_bound(X, g, K_REAL, idx, found, d2)
        print("%s: %d rows' sets differ from the float64 sets; largest excess %.3g of its bound" % (name, differ, worst))
        assert not fails, fails[:3]
        ok = found > 0
        mean = np.array([np.sqrt(d2[n, :found[n]].astype(np.float64)).sum() / max(found[n], 1) for n in range(len(X))])
        assert np.allclose(typ[ok], 1.0 / (mean[ok] + 1e-5), rtol=1e-6) and (typ[~ok] == 0).all()


def test_non_finite_rows(gpu):
    """a NaN row and a +inf row: no neighbours, nobody's neighbour, typicality 0; the others' lists as if those rows were absent"""
    N, D, K = 200, 33, 20
    X = int_rows(N, D)
    keep = np.ones(N, bool)
    keep[[5, 150]] = False
    X[5, 7] = np.nan
    X[150, 32] = np.inf
    idx, d2, found, typ = _run(X, K)
    _check_against_host(X, K, None, (idx, d2, found, typ))
    assert found[[5, 150]].tolist() == [0, 0] and typ[[5, 150]].tolist() == [0, 0] and (idx[[5, 150]] == -1).all()
    assert not np.isin(idx, [5, 150]).any()
    sub = _run(X[keep], K)
    back = np.flatnonzero(keep)
    assert np.array_equal(back[sub[0]], idx[keep]) and np.array_equal(_bits(sub[1]), _bits(d2[keep]))
    assert np.array_equal(_bits(sub[3]), _bits(typ[keep]))


def _argmax_loop(value, group, G):
    best, top = np.full(G, -1, np.int32), np.full(G, -np.inf)
    for n in range(len(value)):
        g = group[n]
        if 0 <= g < G and value[n] > top[g]:
            top[g], best[g] = value[n], n
    return best


@pytest.mark.parametrize("G", [1, 7, 8192])
def test_group_argmax_equals_a_loop(gpu, G):
    from a_link_amd import typiclust
    for N in (1, 255, 256, 257, 5000):
        rng = np.random.RandomState(N + G)
        value = rng.randint(-3, 4, N).astype(np.float32)                   # ties everywhere
        value[rng.random_sample(N) < 0.1] = np.nan
        value[rng.random_sample(N) < 0.1] = -np.inf
        value[rng.random_sample(N) < 0.02] = np.inf
        group = rng.randint(-2, min(G, 12) + 2, N).astype(np.int32)        # out-of-range groups on both sides; with G = 8192: empty groups
        if G == 8192:
            group[rng.random_sample(N) < 0.3] = 8191
            group[rng.random_sample(N) < 0.05] = 8192
        want = _argmax_loop(value, group, G)
        got = typiclust.group_argmax_device(_dev(value), _dev(group), G).cpu().numpy()
        assert np.array_equal(got, want), (N, G)
        assert np.array_equal(typiclust.group_argmax_device(_dev(value), _dev(group), G).cpu().numpy(), got)
    only_bad = np.array([np.nan, -np.inf, np.nan], np.float32)
    assert typiclust.group_argmax_device(_dev(only_bad), _dev(np.zeros(3, np.int32)), 2).cpu().tolist() == [-1, -1]


def _pair_of(X, seed=4):
    """integer tables and indices whose rows |L[li] - R[ri]| are exactly the non-negative integer rows X"""
    rng = np.random.RandomState(seed)
    R = rng.randint(-3, 4, (5, X.shape[1])).astype(np.float32)
    ri = rng.randint(0, 5, len(X)).astype(np.int32)
    L = (X + R[ri]).astype(np.float32)
    perm = rng.permutation(len(X)).astype(np.int32)
    Ls = np.empty_like(L)
    Ls[perm] = L
    return Ls, R, perm, ri


def test_typiclust_device_equals_the_host_on_integer_blobs(gpu):
    from a_link_amd import typiclust
    X, blob, C0 = blobs([30, 20, 12, 4])
    X, C0 = np.abs(X), np.abs(C0)
    lab = np.flatnonzero(blob == 0)[:2]
    L, R, li, ri = _pair_of(X)
    assert np.array_equal(np.abs(L[li] - R[ri]), X)
    for n in (2, 5, 9):                                                    # one round, two, three (three kept clusters)
        want, winfo = typiclust.typiclust(X, lab, n, k_nn=5, centres=C0)
        for rows in (_dev(X), (_dev(L), _dev(R), _dev(li), _dev(ri))):
            got, info = typiclust.typiclust_device(rows, lab, n, k_nn=5, centres=_dev(C0))
            assert np.array_equal(got, want) and got.dtype == np.int64, (n, got, want)
            assert np.array_equal(info["order"], winfo["order"]) and np.array_equal(info["assign"].cpu().numpy(), blob)
            assert np.array_equal(info["typicality"].cpu().numpy(), winfo["typicality"])
    assert winfo["order"].tolist() == [1, 2, 0] and len(set(want.tolist()) & set(lab.tolist())) == 0
    # seeds of its own: the uniforms of the host's RandomState give the host's clusters and picks
    u = np.random.RandomState(6).random_sample(7)
    # (iters = 0: the centres stay integer rows, so both sides assign exactly)
    want, _ = typiclust.typiclust(X, lab, 5, k_nn=5, iters=0, random_state=6)
    got, info = typiclust.typiclust_device(_dev(X), lab, 5, k_nn=5, iters=0, uniforms=u)
    assert np.array_equal(got, want) and info["counts"].numel() == 7
    # the sampler's device route, the labelled rows appended behind the pool
    class Learner(object):
        X_training = X[lab]
    pool = np.delete(X, lab, axis=0)
    idx, inst = typiclust.typiclust_sampling(Learner(), _dev(pool), n_instances=3, k_nn=5, iters=0, random_state=2)
    want, _ = typiclust.typiclust_sampling(Learner(), pool, n_instances=3, k_nn=5, iters=0, random_state=2)
    assert np.array_equal(idx, want) and torch.equal(inst, _dev(pool)[torch.from_numpy(idx).cuda()])


def _committee(D, members=3):
    from a_link_amd import committee, siamese
    return committee.Bagging([siamese.SiameseNetwork((D,), "c%d" % m, 0.1, seed=80 + m) for m in range(members)], [])


def test_bagging_typiclust_indexed_equals_the_module_function(gpu):
    from a_link_amd import typiclust
    X, blob, C0 = blobs([30, 20, 12, 4], D=64)
    X = np.abs(X)
    L, R, li, ri = (_dev(a) for a in _pair_of(X))
    lab = np.flatnonzero(blob == 1)[:3]
    u = np.random.RandomState(1).random_sample(8)
    bag = _committee(64)
    got = bag.typiclust_indexed(L, R, li, ri, lab, 5, k_nn=5, iters=4, uniforms=u)
    want = typiclust.typiclust_device((L, R, li, ri), lab, 5, k_nn=5, iters=4, uniforms=u)
    assert np.array_equal(got[0], want[0]) and len(got[0]) == 5
    assert torch.equal(got[1]["assign"], want[1]["assign"]) and torch.equal(got[1]["typicality"], want[1]["typicality"])
    with pytest.raises(ValueError, match="one feature space"):
        bag.typiclust_indexed([L] * 3, [R] * 3, li, ri, lab, 5)


def test_python_refusals(gpu):
    from a_link_amd import typiclust
    X = _dev(np.random.RandomState(3).randn(50, 8).astype(np.float32))
    g = torch.zeros(50, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="CUDA"):
        typiclust.knn_device(X.cpu(), 4)
    with pytest.raises(ValueError, match="float32"):
        typiclust.knn_device(X.double(), 4)
    for bad in (0, -1, 1.5, 33):
        with pytest.raises(ValueError, match="k = "):
            typiclust.knn_device(X, bad)
    with pytest.raises(ValueError, match="k = 33"):
        typiclust.typicality_device(X, 33)
    with pytest.raises(ValueError, match="empty"):
        typiclust.knn_device(X[:0], 4)
    with pytest.raises(ValueError, match="D = 8200"):
        typiclust.knn_device(torch.zeros((2, 8200), device="cuda"), 1)
    for bad in (g[:49], g.long(), g.cpu(), [0] * 50):
        with pytest.raises(ValueError, match="groups"):
            typiclust.knn_device(X, 4, groups=bad)
    li = _dev(np.arange(4, dtype=np.int32))
    with pytest.raises(ValueError, match="outside its table"):
        typiclust.knn_device((X, X, li + 47, li), 2)
    v = X[:, 0].contiguous()
    with pytest.raises(ValueError, match="value"):
        typiclust.group_argmax_device(v.double(), g, 3)
    with pytest.raises(ValueError, match="group"):
        typiclust.group_argmax_device(v, g[:9], 3)
    for bad in (0, 8193, 2.5):
        with pytest.raises(ValueError, match="n_groups"):
            typiclust.group_argmax_device(v, g, bad)
    run = typiclust.typiclust_device
    with pytest.raises(ValueError, match="empty"):
        run(X[:0], [], 1)
    with pytest.raises(ValueError, match="only 47 of the 50 rows"):
        run(X, [0, 1, 2], 48)
    for bad in ([50], [-1], [1, 1], [0.5]):
        with pytest.raises(ValueError, match="labelled"):
            run(X, bad, 1)
    with pytest.raises(ValueError, match="n_instances"):
        run(X, [], 0)
    with pytest.raises(ValueError, match="k_nn = 40"):
        run(X, [], 2, k_nn=40)
    with pytest.raises(ValueError, match="min_cluster_size"):
        run(X, [], 2, min_cluster_size=-1)


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    x = torch.zeros((8, 4), device="cuda")
    ind = torch.zeros(8, dtype=torch.int32, device="cuda")
    outs = {"idx": torch.full((8, 3), -7, dtype=torch.int32, device="cuda"), "d2": torch.full((8, 3), -7.0, device="cuda"),
            "found": torch.full((8,), -7, dtype=torch.int32, device="cuda"), "typ": torch.full((8,), -7.0, device="cuda")}
    assert lib.alink_knn_scratch_bytes(8, 4, 33) == 0 and lib.alink_knn_scratch_bytes(0, 4, 3) == 0
    assert lib.alink_group_argmax_scratch_bytes(8, 8193) == 0 and lib.alink_group_argmax_scratch_bytes(2 ** 31, 8) == 0
    scratch = torch.empty(max(lib.alink_knn_scratch_bytes(8, 4, 3), lib.alink_group_argmax_scratch_bytes(8, 4)) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(x_=x, r=None, li=None, ri=None, N=8, D=4, K=3, idx=outs["idx"], scratch_ptr=sp, full=True):
        o = [outs[k] if full else None for k in ("d2", "found", "typ")]
        return lib.alink_knn(gpu.ptr(x_), gpu.ptr(r), gpu.ptr(li), gpu.ptr(ri), N, D, None, K, 0, 1e-5, gpu.ptr(idx), gpu.ptr(o[0]), gpu.ptr(o[1]),
                             gpu.ptr(o[2]), C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(x_=None), "NULL"), (dict(idx=None), "NULL"), (dict(scratch_ptr=0), "NULL"),
                     (dict(li=ind), "pair form"), (dict(li=ind, r=x), "pair form"), (dict(li=ind, ri=ind), "pair form"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(D=0), "D=0"), (dict(D=8193), "D=8193"),
                     (dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(scratch_ptr=sp + 4), "aligned")):
        assert call(**kw) == -1, kw                                           # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    best = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    val = torch.zeros(8, device="cuda")

    def amax(v=val, g=ind, N=8, G=4, b=best, scratch_ptr=sp):
        return lib.alink_group_argmax(gpu.ptr(v), gpu.ptr(g), N, G, gpu.ptr(b), C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(v=None), "NULL"), (dict(g=None), "NULL"), (dict(b=None), "NULL"), (dict(scratch_ptr=0), "NULL"),
                     (dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(G=0), "G=0"), (dict(G=8193), "G=8193"),
                     (dict(scratch_ptr=sp + 8), "aligned")):
        assert amax(**kw) == -1, kw
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(K=0), "alink_knn")
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in outs.values()) and bool((best == -7).all())       # a refused call launches nothing
    assert call(full=False) == 0                                              # every output but dev_idx may be NULL
    torch.cuda.synchronize()
    assert outs["idx"].cpu().tolist()[0] == [1, 2, 3] and outs["idx"].cpu().tolist()[7] == [0, 1, 2]
    assert bool((outs["d2"] == -7.0).all()) and bool((outs["found"] == -7).all()) and bool((outs["typ"] == -7.0).all())
    assert call() == 0 and amax() == 0
    torch.cuda.synchronize()
    assert outs["found"].cpu().tolist() == [3] * 8 and bool((outs["d2"] == 0).all()) and best.cpu().tolist() == [0, -1, -1, -1]
