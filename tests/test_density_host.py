"""CPU: information density of a-link_amd/density.py (modAL.density).  modAL is not a dependency: the reference here is a literal
restatement of its two lines.  Also home of the NumPy emulation of alink_information_density's pinned arithmetic and of the
exact inputs that tests/test_gpu_density.py runs on the device: here they are shown to admit no rounding in the sums."""
import functools
import os
import re

import numpy as np
import pytest
from scipy.spatial.distance import euclidean
from sklearn.metrics.pairwise import pairwise_distances

import a_link_amd  # noqa: F401
from a_link_amd import _abi, batch as B, density as Dn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule of include/alink_hip.h in NumPy ---------------------------------------------------------------------------------
def emulate_density(X, Z=None, order=None):
    """-> (density float32 (N,), mean_distance float32 (N,), central, distance sums float64 (N,)).  float32 d2 from direct
    differences (a NumPy row sum: exact — so order-free — on the integer inputs), np.sqrt and a divide in float32, two float64
    sums taken one reference row after the other in `order` (default: ascending), a float64 divide by R, a cast."""
    X = np.ascontiguousarray(X, np.float32)
    Z = X if Z is None else np.ascontiguousarray(Z, np.float32)
    N, R = len(X), len(Z)
    order = np.arange(R) if order is None else np.asarray(order)
    one = np.float32(1)
    sum_s, sum_d = np.zeros(N, np.float64), np.zeros(N, np.float64)
    step = max(1, (1 << 22) // (N * X.shape[1]))
    for j0 in range(0, R, step):
        z = Z[order[j0:j0 + step]]
        d2 = ((X[:, None, :] - z[None, :, :]) ** 2).sum(axis=2, dtype=np.float32)
        d = np.sqrt(d2)
        s = one / (one + d)
        assert d.dtype == np.float32 and s.dtype == np.float32
        for j in range(len(z)):
            sum_s += s[:, j].astype(np.float64)
            sum_d += d[:, j].astype(np.float64)
    central = -1
    best = np.inf
    for n in range(N):                                                       # `<`: the first least sum, a NaN never
        if sum_d[n] < best or (central < 0 and sum_d[n] == best):
            best, central = sum_d[n], n
    return (sum_s / np.float64(R)).astype(np.float32), (sum_d / np.float64(R)).astype(np.float32), central, sum_d


def emulate_ranked(X, Z, u, k, alphas, dtype=np.float32):
    """the ranked-batch rule of include/alink_hip.h (tests/test_gpu_batch.py restates it too), every operation rounded to
    `dtype`, with the weights alpha_t handed in -> (picks, scores, least gap between the best and the second-best score)"""
    X, Z, u = X.astype(dtype), Z.astype(dtype), u.astype(dtype)
    N = len(X)
    one = dtype(1)
    d2 = np.full(N, np.inf, dtype)
    for z in Z:
        d2 = np.minimum(d2, ((X - z) ** 2).sum(axis=1, dtype=dtype))
    picked = np.zeros(N, bool)
    idx, scores, gap = [], [], np.inf
    for t in range(min(k, N)):
        a = dtype(alphas[t])
        score = a * (one - one / (one + np.sqrt(d2))) + (one - a) * u
        score[picked] = -np.inf
        p = int(np.argmax(score))                                            # the first maximum among the rows left
        if N - t > 1:
            gap = min(gap, float(score[p]) - float(np.partition(score, -2)[-2]))
        idx.append(p)
        scores.append(score[p])
        picked[p] = True
        d2 = np.minimum(d2, ((X - X[p]) ** 2).sum(axis=1, dtype=dtype))
    return np.array(idx, np.int32), np.array(scores, dtype), gap


def emulate_cold(X, u, k, dtype=np.float32):
    """the cold ranked batch: the central row, then the rule with that row labelled over the other N - 1 rows with
    alpha_t = (N - 1 - t) / N, indices mapped back -> (picks, scores with NaN first, least score gap)"""
    N = len(X)
    c = emulate_density(X)[2]
    keep = np.r_[0:c, c + 1:N]
    alphas = [np.float32(np.float64(N - 1 - t) / np.float64(N)) for t in range(N)]
    if k > 1 and N > 1:
        idx, sc, gap = emulate_ranked(X[keep], X[c:c + 1], u[keep], k - 1, alphas, dtype)
    else:
        idx, sc, gap = np.zeros(0, np.int32), np.zeros(0, dtype), np.inf
    return np.r_[np.int32(c), keep[idx].astype(np.int32)], np.r_[dtype(np.nan), sc], gap


# ---- the exact inputs: integer features in [-8, 8], D <= 600 (or in {-1, 0, 1} at D = 8192), so that every d2 is an integer
# below 2^24 — exact in float32 in any order — d is 0 or in [1, 2^9), s = fl(1 / fl(1 + d)) lies in [2^-9, 1] and is a
# multiple of 2^-32, and for R <= 2^20 both sums fit in 53 bits: exact in float64 in any order and any grouping.
# (name, N, R or None for the pool itself, D, largest |feature|)
EXACT_SHAPES = [("n_off_32", 777, None, 40, 8), ("registers", 1031, None, 512, 8), ("d_off_4_tiles", 300, 2500, 7, 8),
                ("any_d", 65, None, 600, 8), ("one_row", 1, None, 5, 8), ("one_reference", 33, 1, 8, 8), ("d_limit", 40, None, 8192, 1)]


@functools.lru_cache(maxsize=None)
def exact_case(name):
    """-> (X, Z or None, (density, mean_distance, central, sums) of the emulation): computed once, shared, left unchanged"""
    _, N, R, D, top = [s for s in EXACT_SHAPES if s[0] == name][0]
    rng = np.random.RandomState(1000 + N + D)
    X = rng.randint(-top, top + 1, (N, D)).astype(np.float32)
    Z = None if R is None else rng.randint(-top, top + 1, (R, D)).astype(np.float32)
    want = emulate_density(X, Z)
    for a in (X, Z) + want[:2] + want[3:]:
        if a is not None:
            a.setflags(write=False)
    return X, Z, want


# (N, D, k): the second exhausts the pool
COLD_SHAPES = [(300, 40, 64), (50, 7, 50)]
COLD_SEED = 83


@functools.lru_cache(maxsize=None)
def cold_case(N, D):
    """-> (L, R, li, ri, X, u): integer feature tables in [-4, 4], the rows X = |L[li] - R[ri]| in [0, 8] they form, utilities
    in [0, 1).  (The seed is chosen for the leads that test_cold_inputs_have_no_near_tie asks.)"""
    rng = np.random.RandomState(COLD_SEED + N)
    L, R = rng.randint(-4, 5, (N, D)).astype(np.float32), rng.randint(-4, 5, (N // 2, D)).astype(np.float32)
    li, ri = rng.permutation(N).astype(np.int32), rng.randint(0, N // 2, N).astype(np.int32)
    out = (L, R, li, ri, np.abs(L[li] - R[ri]), rng.rand(N).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- the host module ------------------------------------------------------------------------------------------------------------
def _modal_information_density(X, metric="euclidean"):
    """modAL.density.information_density, restated"""
    similarity_mtx = 1 / (1 + pairwise_distances(X, X, metric=metric))
    return similarity_mtx.mean(axis=1)


def test_information_density_is_modals():
    rng = np.random.RandomState(0)
    X = rng.randn(120, 9)
    got = Dn.information_density(X)
    assert got.dtype == np.float64 and got.shape == (120,)
    assert np.array_equal(got, _modal_information_density(X))
    assert np.array_equal(Dn.information_density(X, "cosine"), _modal_information_density(X, "cosine"))
    assert np.array_equal(Dn.information_density(X, metric="manhattan"), _modal_information_density(X, "manhattan"))
    # pair input is ranked on |left - right|, as batch._rows does
    left, right = rng.randn(120, 9).astype(np.float32), rng.randn(120, 9).astype(np.float32)
    rows = np.abs(left.astype(np.float64) - right.astype(np.float64))
    assert np.array_equal(Dn.information_density([left, right]), _modal_information_density(rows))
    assert np.array_equal(Dn.information_density([left, right], "cosine"), _modal_information_density(rows, "cosine"))
    assert np.array_equal(B._rows([left, right]), rows)
    # what it is for: a row in a cluster is denser than an outlier
    X = np.r_[rng.randn(50, 4) * 0.1, [[9.0, 9.0, 9.0, 9.0]]]
    dens = Dn.information_density(X)
    assert dens[50] == dens.min() and dens[:50].min() > 2 * dens[50]


def test_similarities():
    rng = np.random.RandomState(1)
    a, b = rng.randn(7), rng.randn(7)
    # == 1 / (1 + |a - b|): to the bit where the norm is a number both libraries must hit (3-4-5, 2-3-6-7), and on random
    # vectors to the one or two ulps by which scipy's norm and NumPy's may differ
    for p, q, norm in (([1.0, -2.0], [4.0, 2.0], 5.0), ([0.0, 1.0, 2.0], [2.0, 4.0, 8.0], 7.0), ([3.0], [3.0], 0.0)):
        assert Dn.similarize_distance(euclidean)(np.array(p), np.array(q)) == 1 / (1 + norm)
    assert abs(Dn.similarize_distance(euclidean)(a, b) - 1 / (1 + np.linalg.norm(a - b))) <= 2.0 ** -52
    assert Dn.euclidean_similarity(a, b) == 1 / (1 + euclidean(a, b))
    cos = 1.0 - a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    assert abs(Dn.cosine_similarity(a, b) - 1 / (1 + cos)) < 1e-15
    assert Dn.euclidean_similarity(a, a) == 1.0
    assert Dn.similarize_distance(lambda x, y, scale=1.0: scale * abs(x - y))(1.0, 4.0, scale=2.0) == 1 / 7


def test_density_weighted():
    import torch
    rng = np.random.RandomState(2)
    u, d = rng.rand(30), rng.rand(30) + 0.1
    assert np.array_equal(Dn.density_weighted(u, d, beta=0), u)
    assert np.array_equal(Dn.density_weighted(u, d), u * d) and np.array_equal(Dn.density_weighted(u, d, beta=1.0), u * d)
    assert np.array_equal(Dn.density_weighted(u, d, 2.0), u * d ** 2.0)
    ut, dt = torch.from_numpy(u.astype(np.float32)), torch.from_numpy(d.astype(np.float32))
    assert torch.equal(Dn.density_weighted(ut, dt, beta=0), ut) and torch.equal(Dn.density_weighted(ut, dt, beta=1), ut * dt)


def test_device_forms_check_their_arguments_before_the_gpu():
    """the argument checks that need no device"""
    import torch
    rows, util = torch.zeros(4, 3), torch.zeros(4)
    with pytest.raises(ValueError, match="CUDA"):
        Dn.information_density_device(rows)
    with pytest.raises(ValueError, match="tuple"):
        Dn.information_density_device((rows, rows))
    with pytest.raises(ValueError, match="unknown density output"):
        Dn.information_density_device(rows, want=("median",))
    with pytest.raises(ValueError, match="CUDA"):
        B.ranked_batch_cold_device(rows, util, 2)


def test_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alink_hip.h")).read(), flags=re.S)
    lib = _abi.load()
    for name, ret, nargs in (("alink_information_density_scratch_bytes", "size_t", 1), ("alink_information_density", "int", 13)):
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), header), name
        assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name][1]) == nargs
        assert hasattr(lib, name)
    # scratch: the N float64 distance sums; nothing for an empty call
    assert lib.alink_information_density_scratch_bytes(0) == 0 and lib.alink_information_density_scratch_bytes(-3) == 0
    assert lib.alink_information_density_scratch_bytes(200000) >= 200000 * 8
    assert lib.alink_information_density_scratch_bytes(200001) % 256 == 0


def test_new_kernels_use_no_scratch():
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "density.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    fn, seen = None, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            seen += 1
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
    assert seen == 9, seen                                                    # the sums in eight forms, and the argmin


# ---- the exact inputs admit no rounding in the sums -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in EXACT_SHAPES])
def test_exact_inputs_sum_to_the_same_bits_in_any_order(name):
    """the emulation's float64 sums over the reference rows ascending, and over a random permutation of them: identical bits
    in both outputs and in the sums themselves — so whatever order the kernel adds in, it must give these bits too"""
    X, Z, (dens, mean, central, sums) = exact_case(name)
    R = len(X) if Z is None else len(Z)
    assert R <= 1 << 20
    d2max = X.shape[1] * (2.0 * np.abs(X).max()) ** 2
    assert d2max < 2 ** 24                                                    # every d2 an exact float32 integer
    assert np.sqrt(d2max) < 2 ** 9                                            # d in {0} + [1, 2^9): s a multiple of 2^-32 in [2^-9, 1]
    order = np.random.RandomState(5).permutation(R)
    dens2, mean2, central2, sums2 = emulate_density(X, Z, order)
    assert np.array_equal(_bits(dens2), _bits(dens)) and np.array_equal(_bits(mean2), _bits(mean))
    assert np.array_equal(_bits(sums2), _bits(sums)) and central2 == central
    assert np.array_equal(sums * 2.0 ** 23 % 1, np.zeros(len(X)))            # the distance sums are multiples of 2^-23: nothing was rounded off
    if Z is None:                                                             # the self-pair counts: s = 1, d = 0
        assert (dens >= np.float32(1.0 / R)).all() and central == int(np.argmin(sums))


@pytest.mark.parametrize("N,D,k", COLD_SHAPES)
def test_cold_inputs_have_no_near_tie(N, D, k):
    """the cold cases of the GPU test are compared with the host float64 ranked_batch too, which needs inputs on which float32
    and float64 cannot part ways: the float32 emulation and the float64 one pick the same rows, every pick leads the
    runner-up by more than 1e-5 — on these inputs d2 is exact, so a float32 score (at most 1) carries the roundings of the
    square root, the sum, the division, the difference, two products and a sum, under 8 x 2^-24 = 4.8e-7, and two scores
    can change places only within twice that — the central row leads by more than 1e-3 in the distance sum — and the host ranked_batch with X_training = None gives those picks."""
    L, R, li, ri, X, u = cold_case(N, D)
    idx32, sc32, gap32 = emulate_cold(X, u, k)
    idx64, sc64, gap64 = emulate_cold(X, u, k, np.float64)
    assert np.array_equal(idx32, idx64) and len(set(idx32.tolist())) == min(k, N)
    print("N=%d D=%d: least lead of a pick over the runner-up %.3e (float32), %.3e (float64)" % (N, D, gap32, gap64))
    assert min(gap32, gap64) > 1e-5
    sums = np.sort(exact_sums(X))
    assert sums[1] - sums[0] > 1e-3
    assert np.isnan(sc32[0]) and np.abs(sc32[1:].astype(np.float64) - sc64[1:]).max() < 1e-6

    class _Cold:
        X_training = None
    host = B.ranked_batch(_Cold(), X.astype(np.float64), u.astype(np.float64), k, "euclidean", None)
    assert np.array_equal(host, idx32)
    assert np.array_equal(B.ranked_batch(_Cold(), [L[li], R[ri]], u, k, "euclidean", None), idx32)


def exact_sums(X):
    return pairwise_distances(X.astype(np.float64)).sum(axis=0)
