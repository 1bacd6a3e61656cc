"""CPU: the k-nearest-neighbour rule, typicality and the TypiClust selection of a-link_amd/typiclust.py on the host — against
sklearn's brute-force neighbours and an explicit double loop; the float32 acceptance predicate the GPU test applies to
alink_knn, shown to pass a float32 stand-in of the rule and to fail every mutant of it; the selection on hand-built blobs; and
the compiler's resource report of knn.hip (no kernel may use scratch: the running lists must live in registers)."""
import os
import re

import numpy as np
import pytest

from a_link_amd import _abi, typiclust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_REAL = 20


def int_rows(N, D, seed=0, lo=-4, hi=4):
    """small-integer rows: every product, score and distance is an integer far below 2^24 — exact in any order"""
    return np.random.RandomState(1000 + 7 * N + D + seed).randint(lo, hi + 1, (N, D)).astype(np.float32)


def random_groups(N, G, seed=0, absent=0.1):
    """a random labelling into G groups with some rows of group -1 (and -3: any negative group is nobody's)"""
    rng = np.random.RandomState(2000 + N + G + seed)
    g = rng.randint(0, G, N).astype(np.int32)
    out = rng.random_sample(N) < absent
    g[out] = np.where(rng.random_sample(out.sum()) < 0.5, -1, -3)
    return g


def real_cases():
    """the real-valued inputs of the float32 predicate, here and on the GPU: (name, rows float32, groups or None)"""
    rng = np.random.RandomState(12)
    yield "300 x 128, 3 groups", rng.randn(300, 128).astype(np.float32), random_groups(300, 3)
    yield "260 x 512", (rng.randn(260, 512) * rng.uniform(0.5, 2.0, (260, 1))).astype(np.float32), None


def brute_force(X, k, groups=None):
    """the double loop: per row the (d2, index) pairs of its candidates, sorted -> (idx, d2, found)"""
    X = np.asarray(X, np.float64)
    N = len(X)
    g = np.zeros(N, np.int64) if groups is None else np.asarray(groups)
    idx, d2, found = np.full((N, k), -1, np.int32), np.full((N, k), np.nan), np.zeros(N, np.int32)
    for n in range(N):
        cand = sorted((float(((X[n] - X[j]) ** 2).sum()), j) for j in range(N) if j != n and g[n] >= 0 and g[j] == g[n])[:k]
        found[n] = len(cand)
        for p, (d, j) in enumerate(cand):
            idx[n, p], d2[n, p] = j, d
    return idx, d2, found


def same_lists(got, want):
    """(idx, d2, found) equal: integers equal, d2 equal as values with NaN where the other has NaN -> the first that differs"""
    for name, a, b in zip(("idx", "d2", "found"), got, want):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return name
        if name == "d2":
            a, b = a.astype(np.float64), b.astype(np.float64)
            if not (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])):
                return name
        elif not np.array_equal(a, b):
            return name
    return None


def within_float32_bound(X, groups, k, idx, found, d2=None):
    """The acceptance predicate of a float32 neighbour search.  In float64: s(n, j) = |x_j|^2 - 2 x_n . x_j and
    E(n, j) = g (|x_j|^2 + 2 |x_n| |x_j|), g = (D + 8) 2^-24, the bound of a D-term float32 chain (tests/test_gpu_kmeans.py uses
    it for the same chain).  A result passes when, for every row n, found = min(k, candidates), the reported rows are distinct
    candidates, unfilled slots are -1, every reported j and every unreported candidate i satisfy
    s(n, j) <= s(n, i) + E(n, j) + E(n, i), consecutive entries of a list satisfy the same, and (given d2) each distance lies
    within g of the float64 one.  No row is exempt.
    -> (failures: list of str, rows whose set differs from the float64 set, largest excess as a fraction of its bound)"""
    X = np.asarray(X, np.float64)
    N, D = X.shape
    gr = np.zeros(N, np.int64) if groups is None else np.asarray(groups, np.int64)
    g = (D + 8) * 2.0 ** -24
    sq = (X * X).sum(axis=1)
    norm = np.sqrt(sq)
    S = sq[None, :] - 2.0 * (X @ X.T)
    E = g * (sq[None, :] + 2.0 * norm[:, None] * norm[None, :])
    fails, differ, worst = [], 0, -np.inf                  # (worst < 0: even the closest pair stands in the float64 order)
    for n in range(N):
        cand = np.flatnonzero((gr == gr[n]) & (gr[n] >= 0) & (np.arange(N) != n))
        f = int(found[n])
        rep = np.asarray(idx[n, :f], np.int64)
        if f != min(k, len(cand)):
            fails.append("row %d: found %d of min(%d, %d)" % (n, f, k, len(cand)))
            continue
        if (np.asarray(idx[n, f:]) != -1).any():
            fails.append("row %d: an unfilled slot is not -1" % n)
        if len(set(rep.tolist())) != f or not set(rep.tolist()) <= set(cand.tolist()):
            fails.append("row %d: reports a row twice or a row that is no candidate" % n)
            continue
        true = cand[np.argsort(S[n, cand], kind="stable")[:f]]
        differ += set(true.tolist()) != set(rep.tolist())
        rest = np.setdiff1d(cand, rep)
        if f and rest.size:
            excess = (S[n, rep] - E[n, rep])[:, None] - (S[n, rest] + E[n, rest])[None, :]
            room = E[n, rep][:, None] + E[n, rest][None, :]
            frac = ((S[n, rep][:, None] - S[n, rest][None, :]) / room).max()
            worst = max(worst, frac)
            if (excess > 0).any():
                fails.append("row %d: reports a row %.3g bounds behind one it leaves out" % (n, frac))
        if f > 1:
            step = S[n, rep[:-1]] - S[n, rep[1:]]
            room = E[n, rep[:-1]] + E[n, rep[1:]]
            worst = max(worst, (step / room).max())
            if (step > room).any():
                fails.append("row %d: list out of order by %.3g bounds" % (n, (step / room).max()))
        if d2 is not None and f:
            own = ((X[n] - X[rep]) ** 2).sum(axis=1)
            if not (np.abs(np.asarray(d2[n, :f], np.float64) - own) <= g * own + 1e-30).all():
                fails.append("row %d: a distance off its float64 value by more than g" % n)
    return fails, differ, worst


def standin(X, k, groups=None, mutant=None):
    """a NumPy float32 stand-in of alink_knn's score — a GEMM-form dot in BLAS's summation order, not the kernel's chain — and,
    with `mutant`, one wrong kernel: 'self' (self not excluded), 'kth' (the k-th neighbour replaced by the one two ranks behind),
    'tile' (the last tile of 128 candidates never looked at), 'groups' (groups ignored), 'ties' (ties to the higher index)
    -> (idx int32 (N, k), found int32 (N,))"""
    X = np.asarray(X, np.float32)
    N = len(X)
    gr = np.zeros(N, np.int64) if groups is None else np.asarray(groups, np.int64)
    score = ((X * X).sum(axis=1)[None, :] - np.float32(2) * (X @ X.T)).astype(np.float32)
    ok = (gr[:, None] >= 0) & (gr[None, :] >= 0)
    if mutant != "groups":
        ok &= gr[:, None] == gr[None, :]
    if mutant != "self":
        ok &= ~np.eye(N, dtype=bool)
    if mutant == "tile":
        ok[:, 128 * ((N - 1) // 128):] = False
    score = np.where(ok, score, np.float32(np.inf))
    if mutant == "ties":
        order = (N - 1 - np.argsort(score[:, ::-1], axis=1, kind="stable"))
    else:
        order = np.argsort(score, axis=1, kind="stable")
    if mutant == "kth":
        order = np.concatenate([order[:, :k - 1], order[:, k + 1:k + 2], order[:, k - 1:k + 1], order[:, k + 2:]], axis=1)
    w = min(k, N)
    real = np.take_along_axis(score, order[:, :w], axis=1) < np.inf
    idx = np.full((N, k), -1, np.int32)
    idx[:, :w] = np.where(real, order[:, :w], -1)
    return idx, real.sum(axis=1).astype(np.int32)


# ---- 1. the host rule against brute force ----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,k", [(200, 16, 7), (150, 64, 20), (40, 5, 39)])
def test_host_knn_equals_sklearns_brute_force_on_tie_free_rows(N, D, k):
    from sklearn.neighbors import NearestNeighbors
    X = np.random.RandomState(N).randn(N, D)
    idx, d2, found = typiclust.knn(X, k)
    dist, ind = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(X).kneighbors(X)
    assert np.array_equal(ind[:, 0], np.arange(N))                         # a row is its own nearest: left out on our side
    assert np.array_equal(idx, ind[:, 1:]) and (found == k).all()
    assert np.allclose(np.sqrt(d2), dist[:, 1:], rtol=1e-9, atol=1e-12)
    assert (np.diff(d2, axis=1) >= 0).all()


@pytest.mark.parametrize("N,D,k,G", [(60, 3, 5, None), (90, 2, 20, 3), (33, 1, 32, 1), (70, 4, 8, 40), (5, 6, 9, None)])
def test_host_knn_equals_the_double_loop_on_integer_rows_with_ties(N, D, k, G):
    X = int_rows(N, D, lo=-2, hi=2)
    g = None if G is None else random_groups(N, G)
    got, want = typiclust.knn(X, k, g), brute_force(X, k, g)
    assert same_lists(got, want) is None, same_lists(got, want)
    d2 = want[1]
    if G != 40 and N > 5:                                                  # (40 groups: lists of a row or two; 5 rows: K > N)
        ties = int((d2[:, 1:] == d2[:, :-1]).sum())
        assert ties > N // 2, ties                                         # the case is about ties
    typ = typiclust.typicality(X, k, g)
    for n in range(N):
        f = want[2][n]
        m = 0.0
        for p in range(f):                                                 # ascending slot order
            m += float(np.sqrt(d2[n, p]))
        assert typ[n] == (np.float32(1.0 / (m / f + 1e-5)) if f else 0)
    sq = typiclust.typicality(X, k, g, squared=True, eps=0.5)
    n = int(np.argmax(want[2]))
    assert sq[n] == np.float32(1.0 / (d2[n, :want[2][n]].sum() / want[2][n] + 0.5))


def test_host_knn_rows_without_neighbours():
    X = np.array([[0., 0.], [np.nan, 0.], [3., 0.], [np.inf, 1.], [1., 0.], [1e30, 0.]], np.float32)
    idx, d2, found = typiclust.knn(X, 2)
    assert found.tolist() == [2, 0, 2, 0, 2, 0]                            # NaN, +inf and a norm beyond float32: dead rows
    assert idx.tolist() == [[4, 2], [-1, -1], [4, 0], [-1, -1], [0, 2], [-1, -1]]
    assert np.isnan(d2[[1, 3, 5]]).all() and d2[0].tolist() == [1.0, 9.0]
    assert typiclust.typicality(X, 2)[[1, 3, 5]].tolist() == [0, 0, 0]
    g = np.array([0, 0, 0, 0, -1, 0], np.int32)
    idx, _, found = typiclust.knn(X, 2, g)
    assert idx.tolist()[0] == [2, -1] and found.tolist() == [1, 0, 1, 0, 0, 0]
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="k ="):
            typiclust.knn(X, bad)
    with pytest.raises(ValueError, match="groups"):
        typiclust.knn(X, 2, np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="rows"):
        typiclust.knn(np.zeros((0, 3)), 2)


# ---- 2. the float32 acceptance predicate -----------------------------------------------------------------------------------
def test_the_float32_predicate_passes_a_stand_in_and_fails_every_mutant():
    for name, X, g in real_cases():
        idx, found = standin(X, K_REAL, g)
        fails, differ, worst = within_float32_bound(X, g, K_REAL, idx, found)
        print("%s: the float32 stand-in differs from the float64 sets in %d rows, largest excess %.3g of its bound" % (name, differ, worst))
        assert not fails, fails[:3]
        assert worst <= 1.0
        for mutant in ("self", "kth", "tile") + (("groups",) if g is not None else ()):
            midx, mfound = standin(X, K_REAL, g, mutant)
            moved = float((midx != idx).any(axis=1).mean())
            mfails, _, _ = within_float32_bound(X, g, K_REAL, midx, mfound)
            print("%s: mutant %-6s moves %.1f %% of the rows; the predicate names %d" % (name, mutant, 100 * moved, len(mfails)))
            assert moved > 0 and mfails, mutant
    # ties to the higher index: only exact ties show it, and there the check is equality
    X = int_rows(257, 3, lo=-2, hi=2)
    want = typiclust.knn(X, K_REAL)
    idx, found = standin(X, K_REAL)
    assert np.array_equal(idx, want[0]) and np.array_equal(found, want[2])
    midx, _ = standin(X, K_REAL, mutant="ties")
    moved = float((midx != idx).any(axis=1).mean())
    print("integer rows: mutant ties   moves %.1f %% of the rows" % (100 * moved))
    assert moved > 0.5


# ---- 3. the selection ------------------------------------------------------------------------------------------------------
def blobs(sizes, D=8, seed=3):
    """integer blobs: blob b has sizes[b] rows around 64 e_b with jitter in {-1, 0, 1}, shuffled
    -> (rows float32, blob of each row, one row of each blob as centres)"""
    rng = np.random.RandomState(seed)
    blob = np.repeat(np.arange(len(sizes)), sizes)
    X = np.zeros((len(blob), D))
    X[np.arange(len(blob)), blob % D] = 64
    X += rng.randint(-1, 2, X.shape)
    perm = rng.permutation(len(blob))
    X, blob = X[perm].astype(np.float32), blob[perm]
    C0 = np.stack([X[np.flatnonzero(blob == b)[0]] for b in range(len(sizes))])
    return X, blob, C0


def ranked(typ, rows):
    """`rows` by typicality descending, ties to the lower row"""
    rows = np.sort(np.asarray(rows))
    return rows[np.argsort(-typ[rows].astype(np.float64), kind="stable")]


def test_typiclust_selection_on_integer_blobs():
    X, blob, C0 = blobs([30, 20, 12, 4])
    lab = np.flatnonzero(blob == 0)[:1]                                    # the largest blob is covered
    picks, info = typiclust.typiclust(X, lab, 2, k_nn=5, centres=C0)
    assert np.array_equal(info["assign"], blob) and info["counts"].tolist() == [30, 20, 12, 4]
    assert info["order"].tolist() == [1, 2, 0]                             # uncovered by size; the covered one last; 4 <= 5 rows: dropped
    typ = info["typicality"]
    assert np.array_equal(typ, typiclust.typicality(X, 5, groups=blob))
    assert picks.tolist() == [ranked(typ, np.flatnonzero(blob == 1))[0], ranked(typ, np.flatnonzero(blob == 2))[0]]
    # two rounds: every kept cluster once, then the second most typical rows; the labelled row is never picked
    picks, _ = typiclust.typiclust(X, lab, 5, k_nn=5, centres=C0)
    free0 = np.setdiff1d(np.flatnonzero(blob == 0), lab)
    want = [ranked(typ, np.flatnonzero(blob == 1))[0], ranked(typ, np.flatnonzero(blob == 2))[0], ranked(typ, free0)[0],
            ranked(typ, np.flatnonzero(blob == 1))[1], ranked(typ, np.flatnonzero(blob == 2))[1]]
    assert picks.tolist() == want and lab[0] not in picks and len(set(picks.tolist())) == 5
    # the most typical row of the covered blob labelled: its second takes the place
    top0 = ranked(typ, np.flatnonzero(blob == 0))[:2]
    picks, _ = typiclust.typiclust(X, top0[:1], 3, k_nn=5, centres=C0)
    assert picks[2] == top0[1]
    # nothing kept by min_cluster_size: nothing is dropped
    picks, info = typiclust.typiclust(X, [], 4, k_nn=5, min_cluster_size=30, centres=C0)
    assert info["order"].tolist() == [0, 1, 2, 3] and blob[picks].tolist() == [0, 1, 2, 3]
    # a small cluster runs dry and is skipped; only dropped clusters left: the call ends with what it has
    picks, _ = typiclust.typiclust(X, [], 66, k_nn=5, centres=C0)
    assert len(picks) == 62 and not (blob[picks] == 3).any() and len(set(picks.tolist())) == 62
    # seeds of its own (k-means++): the number of clusters is labelled + budget, capped
    picks, info = typiclust.typiclust(X, lab, 3, k_nn=5, random_state=0)
    assert len(info["counts"]) == 4 and len(picks) == 3
    assert len(typiclust.typiclust(X, lab, 6, k_nn=5, max_clusters=2, random_state=0)[1]["counts"]) == 2


def test_typiclust_refusals():
    X, blob, C0 = blobs([10, 10])
    with pytest.raises(ValueError, match="only 17 of the 20 rows"):
        typiclust.typiclust(X, [0, 1, 2], 18, centres=C0)
    with pytest.raises(ValueError, match="labelled"):
        typiclust.typiclust(X, [20], 1)
    with pytest.raises(ValueError, match="labelled"):
        typiclust.typiclust(X, [-1], 1)
    with pytest.raises(ValueError, match="twice"):
        typiclust.typiclust(X, [3, 3], 1)
    with pytest.raises(ValueError, match="n_instances"):
        typiclust.typiclust(X, [], 0)
    with pytest.raises(ValueError, match="k ="):
        typiclust.typiclust(X, [], 1, k_nn=0)
    with pytest.raises(ValueError, match="max_clusters"):
        typiclust.typiclust(X, [], 1, max_clusters=0)


class _Learner(object):
    def __init__(self, X_training):
        self.X_training = X_training


def test_typiclust_sampling_appends_the_labelled_rows_behind_the_pool():
    from a_link_amd import existing_al
    assert existing_al.get_strategy_object("typiclust_sampling") is typiclust.typiclust_sampling
    X, blob, _ = blobs([30, 20, 12])
    train = X[blob == 0][:3] + 0                                           # three labelled rows that fall into blob 0
    idx, inst = typiclust.typiclust_sampling(_Learner(train), X, n_instances=2, k_nn=5, random_state=1)
    want, _ = typiclust.typiclust(np.vstack([X, train]), np.arange(len(X), len(X) + 3), 2, k_nn=5, random_state=1)
    assert np.array_equal(idx, want) and np.array_equal(inst, X[idx]) and (idx < len(X)).all()
    R = np.zeros_like(X)
    idx2, inst2 = typiclust.typiclust_sampling(_Learner([train, np.zeros_like(train)]), [X, R], n_instances=2, k_nn=5, random_state=1)
    want2, _ = typiclust.typiclust(np.abs(np.vstack([X, train])), np.arange(len(X), len(X) + 3), 2, k_nn=5, random_state=1)
    assert np.array_equal(idx2, want2) and np.array_equal(inst2[0], X[idx2]) and np.array_equal(inst2[1], X[idx2])
    idx3, _ = typiclust.typiclust_sampling(_Learner(None), X, n_instances=3, k_nn=5, random_state=1)
    assert len(idx3) == 3


# ---- 4. the build's resource report ----------------------------------------------------------------------------------------
def test_no_knn_kernel_spills_to_scratch():
    """the running lists of kn_list_kernel are register arrays that only constant indices reach; one index computed at run time
    would move them to scratch memory, silently and at several times the cost.  The build keeps the compiler's per-kernel
    report beside the object (a-link_amd/lib/obj/knn.usage)."""
    if not os.path.exists(_abi.LIB_PATH):
        pytest.skip("the library has not been built: run __graft_entry__.build() first")
    path = os.path.join(ROOT, "a-link_amd", "lib", "obj", "knn.usage")
    assert os.path.exists(path), "build with the Makefile (it writes %s)" % path
    fn, seen, lists = None, 0, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            fn = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and fn and "kernel" in fn:
            seen += 1
            lists += "kn_list_kernel" in fn
            assert int(m.group(1)) == 0, "%s uses %s bytes of scratch per lane" % (fn, m.group(1))
    assert seen >= 20 and lists == 12, (seen, lists)
