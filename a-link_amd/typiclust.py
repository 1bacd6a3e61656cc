"""typiclust — k-nearest-neighbour typicality and TypiClust queries (Hacohen, Dekel & Weinshall 2022, "Active Learning on a Budget:
Opposite Strategies Suit High and Low Budgets").  EXTENSION: the reference imports its strategies from modAL,
which has no such sampler; no reference driver names these.

Every other strategy of this package needs a trained scorer or a labelled set to push against; with a few dozen labelled pairs
and a pool of 10^5 rows, uncertainty-driven queries do worse than random.  TypiClust needs neither: cluster the pool into
(labelled + budget) clusters, go to the largest clusters no labelled row covers yet, and query each one's most TYPICAL row — the
one with the least mean distance to its k nearest neighbours.

The neighbour rule (include/alink_hip.h, alink_knn, states it in full):

    candidates  of row n: every j != n of the same group (`groups`, None: one group); a row of group < 0 has no neighbours and is
                nobody's neighbour, and so has a row whose squared norm is NaN or +inf in float32; duplicates are neighbours at 0
    score       score(n, j) = |x_j|^2 - 2 x_n . x_j  (= d2(n, j) - |x_n|^2: the same order as the distance, one product cheaper);
                a score that is NaN or +inf never enters a list
    list        the k candidates of least (score, index), in that order: ties go to the lower index; `found` of them exist,
                unfilled slots hold index -1 and d2 NaN
    distance    d2 = |x_n - x_j|^2 by direct differences, for the winners only.  A list is in the SCORE's order: on real-valued
                rows score + |x_n|^2 and d2 round differently, so neighbours that tie to the last bit may stand in d2's reverse order
    typicality  1 / (mean over the found neighbours of sqrt(d2) + eps), rounded to float32 once; 0 for a row without neighbours.
                squared=True takes the mean of d2 itself — what the public TypiClust code computes, whose index returns squared
                distances; the default is the paper's formula

`knn`, `typicality` and `typiclust` are that rule in host float64 NumPy (an N x N matrix: small pools only); `knn_device`,
`typicality_device` and `typiclust_device` are alink_knn and alink_group_argmax (knn.hip: the N x N scores on the matrix cores,
never in memory, each lane's k best in registers).  Where nothing rounds, as on small-integer rows, the two agree bit for bit.

The selection rule of `typiclust` / `typiclust_device`:

    1. `labelled` are row indices into `rows`: labelled and unlabelled rows are clustered together.
    2. The number of clusters is min(len(labelled) + n_instances, max_clusters, cluster.MAX_K) (with `centres`: their number).
    3. cluster.kmeans from badge.kmeans_pp's seeds, `iters` updates.
    4. Typicality with groups = the final assignment: a row's neighbours lie in its own cluster.
    5. Clusters of at most min_cluster_size rows are dropped; if that drops every cluster, none is dropped.
    6. The rest are ordered by (labelled rows in the cluster ascending, size descending, id ascending).
    7. Pick i comes from cluster order[i mod len(order)]: its row of largest typicality among the rows neither labelled nor
       picked, ties to the lower row.  (One round of len(order) picks is one alink_group_argmax on the device.)
    8. A cluster with no such row is skipped; a whole round without a pick ends the call with the picks so far (what is left
       lies in dropped clusters).
    9. Fewer than n_instances rows that are not labelled raises ValueError before anything runs.

Deliberate difference from the public implementation: that code shrinks k to half the cluster size for small clusters; here the
mean runs over min(k, found) neighbours — in a cluster of c rows, over its other c - 1 rows when c - 1 < k.
Queries against a separate reference set: cal.knn_rect / cal.knn_rect_device.  Not built: k > 32, a cosine metric, several
ranks' pools in one call, skipping candidate tiles that hold no row of a workgroup's groups.
"""
import numpy as np

from . import badge as _badge
from . import cluster as _cluster
from .batch import _rows

MAX_K_NN = 32                                              # neighbours of a device call (KN_MAX_K, knn.hip)
MAX_GROUPS = 8192                                          # groups of a device argmax (KN_MAX_G, knn.hip)


def _check_k(k):
    if int(k) != k or int(k) < 1:
        raise ValueError("k = %r must be an integer >= 1" % (k,))
    return int(k)


def _groups_host(groups, N):
    if groups is None:
        return np.zeros(N, np.int64)
    g = np.asarray(groups)
    if g.shape != (N,) or g.dtype.kind not in "iu":
        raise ValueError("groups: %d integers are needed (got shape %s, %s)" % (N, g.shape, g.dtype))
    return g.astype(np.int64)


def knn(rows, k, groups=None):
    """The k nearest neighbours of every row of the (N, D) array `rows` among the other rows of its group, on the host: the rule
    of the module docstring in float64.  EXTENSION.  -> (idx int32 (N, k), d2 float64 (N, k), found int32 (N,))."""
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    k = _check_k(k)
    N = X.shape[0]
    g = _groups_host(groups, N)
    with np.errstate(invalid="ignore", over="ignore"):
        norms = (X * X).sum(axis=1)
        alive = (g >= 0) & np.isfinite(norms.astype(np.float32))
        score = norms[None, :] - 2.0 * (X @ X.T)
        ok = alive[:, None] & alive[None, :] & (g[:, None] == g[None, :]) & ~np.eye(N, dtype=bool) & (score < np.inf)
        score = np.where(ok, score, np.inf)
    w = min(k, N)
    order = np.argsort(score, axis=1, kind="stable")[:, :w]                 # ties to the lower index
    real = np.take_along_axis(score, order, axis=1) < np.inf
    idx = np.full((N, k), -1, np.int32)
    idx[:, :w] = np.where(real, order, -1)
    d2 = np.full((N, k), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        d2[:, :w] = np.where(real, ((X[:, None, :] - X[order]) ** 2).sum(axis=2), np.nan)
    return idx, d2, real.sum(axis=1).astype(np.int32)


def _typicality_of(d2, found, squared, eps):
    d = np.where(np.isnan(d2), 0.0, d2 if squared else np.sqrt(np.where(np.isnan(d2), 0.0, d2)))
    total = np.zeros(len(d))
    for p in range(d.shape[1]):                                            # ascending slot order
        total = total + d[:, p]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(found > 0, 1.0 / (total / np.maximum(found, 1) + float(eps)), 0.0).astype(np.float32)


def typicality(rows, k=20, groups=None, squared=False, eps=1e-5):
    """The typicality of every row on the host: float32(1 / (mean distance to its min(k, found) nearest neighbours + eps)), 0 for a
    row without neighbours.  EXTENSION.  squared=True: the mean of the squared distances (the public TypiClust code's number)."""
    _, d2, found = knn(rows, k, groups)
    return _typicality_of(d2, found, squared, eps)


def _labelled_indices(labelled, N):
    lab = np.asarray([] if labelled is None else labelled)
    if lab.size == 0:
        return np.zeros(0, np.int64)
    if lab.ndim != 1 or lab.dtype.kind not in "iu":
        raise ValueError("labelled: a 1-D array of row indices is needed (got shape %s, %s)" % (lab.shape, lab.dtype))
    lab = lab.astype(np.int64)
    if lab.min() < 0 or lab.max() >= N:
        raise ValueError("labelled: a row index outside 0 .. %d" % (N - 1))
    if len(np.unique(lab)) != len(lab):
        raise ValueError("labelled: a row index is named twice")
    return lab


def _plan(N, labelled, n_instances, k_nn, min_cluster_size, max_clusters, n_centres):
    """the checks every route makes before anything runs -> (labelled int64, n, k_nn, clusters)"""
    n = _cluster._check_instances(n_instances)
    k_nn = _check_k(k_nn)
    if int(min_cluster_size) != min_cluster_size or int(min_cluster_size) < 0:
        raise ValueError("min_cluster_size = %r must be an integer >= 0" % (min_cluster_size,))
    if int(max_clusters) != max_clusters or int(max_clusters) < 1:
        raise ValueError("max_clusters = %r must be an integer >= 1" % (max_clusters,))
    lab = _labelled_indices(labelled, N)
    if N - len(lab) < n:
        raise ValueError("n_instances = %d but only %d of the %d rows are not labelled" % (n, N - len(lab), N))
    K = n_centres if n_centres is not None else min(len(lab) + n, int(max_clusters), _cluster.MAX_K)
    return lab, n, k_nn, K


def _cluster_order(counts, labelled_counts, min_cluster_size):
    """steps 5 and 6 of the selection rule -> the cluster ids in visiting order"""
    keep = np.flatnonzero(counts > int(min_cluster_size))
    if keep.size == 0:
        keep = np.arange(len(counts))
    return sorted(keep.tolist(), key=lambda j: (int(labelled_counts[j]), -int(counts[j]), j))


def _group_argmax_host(value, group, G):
    best = np.full(G, -1, np.int64)
    top = np.full(G, -np.inf)
    for n in range(len(value)):
        g = group[n]
        if 0 <= g < G and value[n] > top[g]:
            top[g], best[g] = value[n], n
    return best


def typiclust(rows, labelled, n_instances, k_nn=20, min_cluster_size=5, max_clusters=500, iters=10, centres=None, random_state=None):
    """TypiClust on the host: n_instances queries among the rows of the (N, D) array `rows` that `labelled` does not name, by the
    selection rule of the module docstring, everything in float64 NumPy.  EXTENSION.

    centres       None: badge.kmeans_pp's seeds with np.random.RandomState(random_state)'s uniforms; else (K, D) initial centres
    -> (picks int64, info): the picks in order (fewer than n_instances only by rule 8); info: kmeans' dict with "typicality"
    (float32 (N,)) and "order" (the visiting order of the clusters) beside it."""
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    N = X.shape[0]
    lab, n, k_nn, K = _plan(N, labelled, n_instances, k_nn, min_cluster_size, max_clusters, None if centres is None else len(centres))
    if centres is None:
        seeds, _ = _badge.kmeans_pp(X, K, np.random.RandomState(random_state).random_sample(K))
        centres = np.full((K, X.shape[1]), np.inf, np.float32)
        centres[seeds >= 0] = X[seeds[seeds >= 0]]
    info = _cluster.kmeans(X, centres, iters)
    assign = info["assign"]
    typ = typicality(X, k_nn, groups=assign)
    order = _cluster_order(info["counts"], np.bincount(assign[lab][assign[lab] >= 0], minlength=K), min_cluster_size)
    value = typ.astype(np.float64)
    value[lab] = -np.inf
    picks = []
    while len(picks) < n:
        best = _group_argmax_host(value, assign, K)[order]
        best = best[best >= 0][:n - len(picks)]
        if best.size == 0:
            break
        picks.extend(best.tolist())
        value[best] = -np.inf
    info["typicality"], info["order"] = typ, np.asarray(order, np.int64)
    return np.asarray(picks, np.int64), info


# ---- device forms -------------------------------------------------------------------------------------------------------------
def _knn_call(rows, k, groups, squared, eps, want_typicality):
    import torch
    from . import _abi, net_host
    from .batch import _pool_rows
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if N < 1:
        raise ValueError("knn_device: the pool is empty")
    if D > _cluster.MAX_D:
        raise ValueError("rows have D = %d columns, beyond the %d a device row may have" % (D, _cluster.MAX_D))
    k = _check_k(k)
    if k > MAX_K_NN:
        raise ValueError("k = %d beyond the %d neighbours a device call keeps" % (k, MAX_K_NN))
    if groups is not None:
        if not isinstance(groups, torch.Tensor) or groups.device != dev or groups.dtype is not torch.int32 or groups.shape != (N,):
            raise ValueError("groups: an int32 tensor of %d values on the pool's device is needed" % N)
        groups = groups.contiguous()
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_knn_scratch_bytes(N, D, k), dev)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((N, k), dtype=torch.float32, device=dev)
    found = torch.empty(N, dtype=torch.int32, device=dev)
    typ = torch.empty(N, dtype=torch.float32, device=dev) if want_typicality else None
    _abi.check(lib.alink_knn(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(groups), k, 1 if squared else 0,
                             float(eps), _abi.ptr(idx), _abi.ptr(d2), _abi.ptr(found), _abi.ptr(typ), sp, _abi.current_stream(dev)),
               "alink_knn")
    return idx, d2, found, typ


def knn_device(rows, k, groups=None):
    """The k nearest neighbours of every pool row on the GPU (alink_knn).  EXTENSION.

    rows    the pool as in cluster.kmeans_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri)
    k       1 .. 32
    groups  None, or CUDA int32 (N,): neighbours only within a group, rows of group < 0 left out (cluster.kmeans_device's "assign")
    -> (idx int32 (N, k), d2 float32 (N, k), found int32 (N,)) on the device.  Nothing is synchronised or read back except, in the
    pair form, the range check of li / ri."""
    return _knn_call(rows, k, groups, False, 0.0, False)[:3]


def typicality_device(rows, k=20, groups=None, squared=False, eps=1e-5):
    """The typicality of every pool row on the GPU (alink_knn): rows, k, groups as in knn_device; squared, eps as in typicality.
    EXTENSION.  -> float32 (N,) on the device."""
    return _knn_call(rows, k, groups, squared, eps, True)[3]


def group_argmax_device(value, group, n_groups):
    """Per group 0 .. n_groups - 1 the row of largest value (alink_group_argmax): `>` from -inf, ties to the lower row, NaN and -inf
    never win, -1 for a group without a winner.  EXTENSION.  value CUDA float32 (N,), group CUDA int32 (N,).  -> int32 (n_groups,)."""
    import torch
    from . import _abi, net_host
    if not isinstance(value, torch.Tensor) or not value.is_cuda or value.dtype is not torch.float32 or value.dim() != 1:
        raise ValueError("value: a 1-D CUDA float32 tensor is needed")
    N, dev = value.numel(), value.device
    if N < 1:
        raise ValueError("group_argmax_device: no rows")
    if not isinstance(group, torch.Tensor) or group.device != dev or group.dtype is not torch.int32 or group.shape != (N,):
        raise ValueError("group: an int32 tensor of %d values on the values' device is needed" % N)
    if int(n_groups) != n_groups or not 1 <= int(n_groups) <= MAX_GROUPS:
        raise ValueError("n_groups = %r outside 1 .. %d" % (n_groups, MAX_GROUPS))
    G = int(n_groups)
    value, group = value.contiguous(), group.contiguous()
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_group_argmax_scratch_bytes(N, G), dev)
    best = torch.empty(G, dtype=torch.int32, device=dev)
    _abi.check(lib.alink_group_argmax(_abi.ptr(value), _abi.ptr(group), N, G, _abi.ptr(best), sp, _abi.current_stream(dev)),
               "alink_group_argmax")
    return best


def typiclust_device(rows, labelled, n_instances, k_nn=20, min_cluster_size=5, max_clusters=500, iters=10, centres=None, uniforms=None,
                     seed=None):
    """TypiClust on the GPU: the selection rule of the module docstring with cluster.kmeans_device (seeds: badge.kmeans_pp_device
    with `uniforms` / `seed`, or `centres`), typicality_device inside the clusters and one group_argmax_device per round.  EXTENSION.

    rows      the pool as in knn_device; labelled: host integers, row indices into it
    -> (picks int64 NumPy array, info): info is kmeans_device's dict with "typicality" (float32 (N,), device) and "order" beside it.
    Read back: the K-sized tables (counts, the labelled rows' clusters) once, and each round's K winners."""
    import torch
    from .batch import _pool_rows
    N, dev = _pool_rows(rows, torch)[4::2]
    if N < 1:
        raise ValueError("typiclust_device: the pool is empty")
    lab, n, k_nn, K = _plan(N, labelled, n_instances, k_nn, min_cluster_size, max_clusters, None if centres is None else len(centres))
    if k_nn > MAX_K_NN:
        raise ValueError("k_nn = %d beyond the %d neighbours a device call keeps" % (k_nn, MAX_K_NN))
    info = _cluster.kmeans_device(rows, K, iters=iters, centres=centres, uniforms=uniforms, seed=seed)
    assign = info["assign"]
    typ = typicality_device(rows, k_nn, groups=assign)
    lab_dev = torch.from_numpy(lab).to(dev)
    lab_assign = assign.index_select(0, lab_dev).cpu().numpy()
    order = _cluster_order(info["counts"].cpu().numpy(), np.bincount(lab_assign[lab_assign >= 0], minlength=K), min_cluster_size)
    value = typ.clone()
    value[lab_dev] = float("-inf")
    picks = []
    while len(picks) < n:
        best = group_argmax_device(value, assign, K).cpu().numpy().astype(np.int64)[order]
        best = best[best >= 0][:n - len(picks)]
        if best.size == 0:
            break
        picks.extend(best.tolist())
        value[torch.from_numpy(best).to(dev)] = float("-inf")
    info["typicality"], info["order"] = typ, np.asarray(order, np.int64)
    return np.asarray(picks, np.int64), info


def typiclust_sampling(classifier, X, n_instances=1, k_nn=20, min_cluster_size=5, max_clusters=500, iters=10, random_state=None):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=typiclust_sampling)): TypiClust queries among the rows of X, an
    (N, D) array or pair input [left, right] (rows |left - right|).  EXTENSION.  The learner's labelled rows (`classifier.X_training`,
    as batch.uncertainty_batch_sampling takes them; None: none) are appended behind the pool and named as `labelled`; the scorer
    itself is not consulted.  CUDA tensors go through typiclust_device, anything else through typiclust.  random_state: the seed of
    the k-means++ uniforms.  -> (query_idx, instances): the instances as the other samplers of this package return them for pair
    input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    training = getattr(classifier, "X_training", None)
    on_device = _cluster._is_cuda(X)
    kw = dict(k_nn=k_nn, min_cluster_size=min_cluster_size, max_clusters=max_clusters, iters=iters)
    if on_device:
        import torch
        rows = (X[0] - X[1]).abs() if isinstance(X, (list, tuple)) else X
        N = rows.shape[0]
        if training is not None:
            if _cluster._is_cuda(training):
                extra = (training[0] - training[1]).abs() if isinstance(training, (list, tuple)) else training
            else:
                extra = torch.from_numpy(_rows(training).astype(np.float32)).to(rows.device)
            rows = torch.cat([rows, extra.to(torch.float32)], dim=0)
        query_idx, _ = typiclust_device(rows, np.arange(N, rows.shape[0]), n_instances, seed=random_state, **kw)
    else:
        rows = _rows(X)
        N = len(rows)
        if training is not None:
            rows = np.vstack([rows, _rows(training)])
        query_idx, _ = typiclust(rows, np.arange(N, len(rows)), n_instances, random_state=random_state, **kw)
    return query_idx, _cluster._instances(X, query_idx, on_device)
