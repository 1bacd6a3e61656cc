"""cluster — the clustering family of diverse batch strategies: k-means over the pool rows, one query per cluster.  EXTENSION
(DESIGN.md §0, X11): the reference imports its strategies from modAL, which has no such sampler; no reference driver names these.

The strategies of this module:

    kmeans_sampling             cluster the rows into k groups and query the row nearest to each centre — the `KMeansSampling`
                                baseline of the BADGE / core-set papers (Ash et al. 2020)
    diverse_minibatch_sampling  diverse mini-batch active learning (Zhdanov 2019): keep the beta * k most informative rows, run
                                k-means on them weighted by informativeness, query the row nearest to each centre

(core-set / farthest-first is batch.ranked_batch_device(alpha=1); BADGE is badge.py, whose k-means++ seeds start Lloyd's
iterations here.)  The rule both share (include/alink_hip.h, alink_kmeans, states it in full):

    assignment  score(n, j) = |c_j|^2 - 2 x_n . c_j;  a_n = argmin_j, ties to the lower j; a score that is NaN or +inf never wins,
                so a centre with a non-finite element stays empty and as it is, and a NaN row has a_n = -1, d2_n = NaN and is left
                out of every sum and count;  d2_n = |x_n - c_(a_n)|^2 by direct differences
    update      c_j <- float32(sum_(a_n = j) w_n x_n / sum_(a_n = j) w_n), the sums in float64; a weight that is not finite and > 0
                counts as 0; a cluster without weight keeps its centre (no relocation)
    schedule    iters times (assign, update), then one last assignment

`kmeans` is that rule in host float64 NumPy; `kmeans_device` is alink_kmeans (kmeans.hip: the assignment on the matrix cores,
fused with its argmin — the (N x K) scores never exist — and float64 updates in a fixed order).  Where nothing rounds, as on
small-integer rows, the two agree bit for bit.  Not built: several ranks' pools in one call, a cosine metric, k > 8192, relocating
empty clusters, mini-batch k-means, an early return once an iteration changes nothing (the remaining passes run and repeat it).
"""
import numpy as np

from . import badge as _badge
from .batch import _rows
from .uncertainty import classifier_uncertainty

MAX_D = 8192                                               # columns of a device row (RB_MAX_D, batch_rows.h)
MAX_K = 8192                                               # clusters of a device call (KM_MAX_K, kmeans.hip)


def _weights_host(weights, N):
    if weights is None:
        return np.ones(N, np.float64)
    w = np.asarray(weights, np.float32).reshape(-1).astype(np.float64)
    if w.size != N:
        raise ValueError("weights: %d values for %d rows" % (w.size, N))
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(w) & (w > 0), w, 0.0)


def _assign_host(X, C):
    """one assignment of the float64 rows X to the float32 centres C -> (assign int32, d2 float64)"""
    Cd = C.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        score = (Cd * Cd).sum(axis=1)[None, :] - 2.0 * (X @ Cd.T)
        score = np.where(score < np.inf, score, np.inf)            # NaN and +inf never win
        a = np.argmin(score, axis=1).astype(np.int32)              # the first of equal minima: ties to the lower centre
        a[~(score[np.arange(len(X)), a] < np.inf)] = -1
        d2 = np.full(len(X), np.nan)
        ok = a >= 0
        d2[ok] = ((X[ok] - Cd[a[ok]]) ** 2).sum(axis=1)
    return a, d2


def kmeans(rows, centres, iters, weights=None):
    """Lloyd's k-means of the (N, D) array `rows` on the host, the rule of the module docstring in float64.  EXTENSION.

    centres  (K, D) initial centres (rounded to float32, as after every update)
    iters    update steps T >= 0; one more assignment follows the last
    weights  None, or N values; one that is not finite and > 0 counts as 0
    -> dict: centres float32 (K, D), assign int32 (N,), d2 float64 (N,), inertia float64 (T + 1,), changed int32 (T + 1,),
    counts int32 (K,), wsum float64 (K,), nearest int32 (K,) — the row of least d2 of each final cluster (ties to the lower row;
    -1 for a cluster without rows)."""
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    C = np.array(centres, np.float32)
    if C.ndim != 2 or C.shape[0] < 1 or C.shape[1] != X.shape[1]:
        raise ValueError("centres: a (K, %d) array with K >= 1 is needed (got shape %s)" % (X.shape[1], C.shape))
    if int(iters) != iters or int(iters) < 0:
        raise ValueError("iters = %r must be an integer >= 0" % (iters,))
    T, (N, _), K = int(iters), X.shape, C.shape[0]
    w = _weights_host(weights, N)
    inertia, changed = np.zeros(T + 1, np.float64), np.zeros(T + 1, np.int32)
    prev = np.full(N, -1, np.int32)
    for t in range(T + 1):
        a, d2 = _assign_host(X, C)
        use = (a >= 0) & (w > 0)
        inertia[t] = (w[use] * d2[use]).sum()
        changed[t] = int((a != prev).sum())
        prev = a
        if t == T:
            break
        for j in range(K):
            m = use & (a == j)
            ws = w[m].sum()
            if ws > 0:
                with np.errstate(invalid="ignore", over="ignore"):
                    C[j] = ((w[m, None] * X[m]).sum(axis=0) / ws).astype(np.float32)
    counts = np.array([(a == j).sum() for j in range(K)], np.int32)
    wsum = np.array([w[a == j].sum() for j in range(K)], np.float64)
    nearest = np.full(K, -1, np.int32)
    for j in range(K):
        m = np.flatnonzero(a == j)
        if m.size:
            nearest[j] = m[np.argmin(d2[m])]
    return {"centres": C, "assign": a, "d2": d2, "inertia": inertia, "changed": changed, "counts": counts, "wsum": wsum,
            "nearest": nearest}


def _check_k_iters(n_clusters, iters):
    if int(n_clusters) != n_clusters or int(n_clusters) < 1:
        raise ValueError("n_clusters = %r must be an integer >= 1" % (n_clusters,))
    if int(n_clusters) > MAX_K:
        raise ValueError("n_clusters = %d beyond the %d a device call takes" % (n_clusters, MAX_K))
    if int(iters) != iters or int(iters) < 0:
        raise ValueError("iters = %r must be an integer >= 0" % (iters,))


def kmeans_device(rows, n_clusters, iters=10, weights=None, centres=None, uniforms=None, seed=None):
    """Lloyd's k-means of a pool on the GPU (alink_kmeans).  EXTENSION.

    rows        the pool as in batch.ranked_batch_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri) —
                row n is |left[li[n]] - right[ri[n]]|, formed on the fly, never materialised
    n_clusters  K in 1 .. 8192 (with `centres`: their number)
    iters       update steps T >= 0; one more assignment follows the last
    weights     None, or CUDA float32 (N,); a weight that is not finite and > 0 counts as 0
    centres     CUDA float32 (K, D) initial centres (copied); None: badge.kmeans_pp_device's min(K, N) seeds with `uniforms` /
                `seed`, the picked rows gathered on the device — a -1 pick (fewer distinct rows than clusters) becomes a centre of
                +inf, which stays empty; with K > N the clusters past N are such centres too
    -> dict of device tensors: centres float32 (K, D), assign int32 (N,), d2 float32 (N,), inertia float64 (T + 1,), changed
    int32 (T + 1,), counts int32 (K,), wsum float64 (K,), nearest int32 (K,).  Nothing is synchronised or read back except, in
    the pair form, the range check of li / ri."""
    import torch
    from . import _abi, net_host
    from .batch import _pool_rows, _f32_matrix, _utility_vector
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if N < 1:
        raise ValueError("kmeans_device: the pool is empty")
    if D > MAX_D:
        raise ValueError("rows have D = %d columns, beyond the %d a device row may have" % (D, MAX_D))
    if centres is not None:
        C = _f32_matrix("centres", centres, torch, dev, D).clone()
        if C.shape[0] < 1:
            raise ValueError("centres: at least one centre is needed")
        n_clusters = C.shape[0]
    _check_k_iters(n_clusters, iters)
    K, T = int(n_clusters), int(iters)
    w = None
    if weights is not None:
        try:
            w = _utility_vector(weights, N, dev, torch)
        except ValueError as e:
            raise ValueError(str(e).replace("utility", "weights"))
    if centres is None:
        k0 = min(K, N)
        idx, _ = _badge.kmeans_pp_device(rows, k0, uniforms=uniforms, seed=seed)
        pick = idx.clamp(min=0).long()
        if li is None:
            seeds = left.index_select(0, pick)
        else:
            seeds = (left.index_select(0, li.index_select(0, pick).long()) - right.index_select(0, ri.index_select(0, pick).long())).abs()
        C = torch.full((K, D), float("inf"), dtype=torch.float32, device=dev)
        C[:k0] = torch.where((idx >= 0).unsqueeze(1), seeds, C[:k0])
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_kmeans_scratch_bytes(N, D, K), dev)
    out = {"centres": C,
           "assign": torch.empty(N, dtype=torch.int32, device=dev), "d2": torch.empty(N, dtype=torch.float32, device=dev),
           "inertia": torch.empty(T + 1, dtype=torch.float64, device=dev), "changed": torch.empty(T + 1, dtype=torch.int32, device=dev),
           "counts": torch.empty(K, dtype=torch.int32, device=dev), "wsum": torch.empty(K, dtype=torch.float64, device=dev),
           "nearest": torch.empty(K, dtype=torch.int32, device=dev)}
    _abi.check(lib.alink_kmeans(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(w), _abi.ptr(C), K, T,
                                _abi.ptr(out["assign"]), _abi.ptr(out["d2"]), _abi.ptr(out["inertia"]), _abi.ptr(out["changed"]),
                                _abi.ptr(out["counts"]), _abi.ptr(out["wsum"]), _abi.ptr(out["nearest"]), sp,
                                _abi.current_stream(dev)), "alink_kmeans")
    return out


def _check_instances(n_instances):
    if int(n_instances) != n_instances or int(n_instances) < 1:
        raise ValueError("n_instances = %r must be at least 1" % (n_instances,))
    return int(n_instances)


def kmeans_sampling_device(rows, n_instances, iters=10, weights=None, uniforms=None, seed=None):
    """k-means sampling of a pool on the GPU: kmeans_device with K = min(n_instances, N) clusters from k-means++ seeds, one query
    per cluster.  EXTENSION.  -> (idx int32 (K,), info): idx = info["nearest"], the row nearest to each final centre (-1 for an
    empty cluster); info is kmeans_device's dict."""
    k = _check_instances(n_instances)
    if isinstance(rows, (tuple, list)):                    # (kmeans_device checks the pool; only its length is needed before)
        N = int(rows[2].numel()) if len(rows) == 4 and hasattr(rows[2], "numel") else 0
    else:
        N = int(rows.shape[0]) if len(getattr(rows, "shape", ())) == 2 else 0
    info = kmeans_device(rows, min(k, N) if N > 0 else k, iters=iters, weights=weights, uniforms=uniforms, seed=seed)
    return info["nearest"], info


def diverse_minibatch_device(rows, utility, n_instances, beta=10, iters=10, uniforms=None, seed=None):
    """Diverse mini-batch active learning (Zhdanov 2019) on the GPU.  EXTENSION.  The min(N, beta * k) rows of largest `utility`
    (uncertainty.topk_device; CUDA float32 (N,), larger = more informative) are clustered into k = min(n_instances, N) groups
    with their utilities as weights (kmeans_device; the pair form passes li[top], ri[top] and copies no features), one query per
    cluster.  -> (idx int32 (k,), info): the row nearest to each final centre as an index into the POOL (-1 for an empty cluster);
    info is kmeans_device's dict over the kept rows, with "top" (int32, their pool indices) beside it."""
    import torch
    from . import uncertainty as _unc
    from .batch import _pool_rows, _utility_vector
    k = _check_instances(n_instances)
    if int(beta) != beta or int(beta) < 1:
        raise ValueError("beta = %r must be an integer >= 1" % (beta,))
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if N < 1:
        raise ValueError("diverse_minibatch_device: the pool is empty")
    utility = _utility_vector(utility, N, dev, torch)
    k = min(k, N)
    top, vals = _unc.topk_device(utility, min(N, int(beta) * k))
    tl = top.long()
    sub = left.index_select(0, tl) if li is None else (left, right, li.index_select(0, tl), ri.index_select(0, tl))
    info = kmeans_device(sub, k, iters=iters, weights=vals, uniforms=uniforms, seed=seed)
    near = info["nearest"]
    idx = torch.where(near >= 0, top.index_select(0, near.clamp(min=0).long()), near)
    info["top"] = top
    return idx, info


def _host_pick(rows, k, iters, random_state, weights=None):
    k = min(k, len(rows))
    seeds, _ = _badge.kmeans_pp(rows, k, np.random.RandomState(random_state).random_sample(k))
    C = np.full((k, rows.shape[1]), np.inf, np.float32)
    C[seeds >= 0] = rows[seeds[seeds >= 0]]
    return kmeans(rows, C, iters, weights=weights)["nearest"]


def _instances(X, query_idx, on_device):
    if on_device:
        import torch
        take = torch.from_numpy(query_idx).to(X[0].device)
        return [X[0][take], X[0][take]] if isinstance(X, (list, tuple)) else X[take]
    return [X[0][query_idx], X[0][query_idx]] if isinstance(X, (list, tuple)) else X[query_idx]


def _is_cuda(X):
    x = X[0] if isinstance(X, (list, tuple)) else X
    return hasattr(x, "is_cuda") and x.is_cuda


def kmeans_sampling(classifier, X, n_instances=1, random_state=None, iters=10):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=kmeans_sampling)): k-means sampling of n_instances rows of X, an
    (N, D) array or pair input [left, right] (rows |left - right|).  EXTENSION.  `classifier` is not consulted.  CUDA tensors go
    through kmeans_sampling_device, anything else through badge.kmeans_pp and kmeans.  random_state: the seed of
    np.random.RandomState for the seeding's uniforms.  -> (query_idx, instances): one pick per non-empty cluster; the instances as
    the other samplers of this package return them for pair input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    k = _check_instances(n_instances)
    on_device = _is_cuda(X)
    if on_device:
        rows = (X[0] - X[1]).abs() if isinstance(X, (list, tuple)) else X
        query_idx = kmeans_sampling_device(rows, k, iters=iters, seed=random_state)[0].cpu().numpy().astype(np.int64)
    else:
        query_idx = _host_pick(_rows(X), k, iters, random_state).astype(np.int64)
    query_idx = query_idx[query_idx >= 0]
    return query_idx, _instances(X, query_idx, on_device)


def diverse_minibatch_sampling(classifier, X, n_instances=1, beta=10, random_state=None, iters=10, **uncertainty_measure_kwargs):
    """modAL-shaped query strategy: a diverse mini-batch (Zhdanov 2019) of n_instances rows of X — the beta * k rows of largest
    classification uncertainty (uncertainty.classifier_uncertainty), clustered with that uncertainty as weight, one query per
    non-empty cluster.  EXTENSION.  X, random_state, the device route and the returned instances as in kmeans_sampling."""
    k = _check_instances(n_instances)
    if int(beta) != beta or int(beta) < 1:
        raise ValueError("beta = %r must be an integer >= 1" % (beta,))
    utility = classifier_uncertainty(classifier, X, **uncertainty_measure_kwargs)
    on_device = _is_cuda(X)
    if on_device:
        import torch
        rows = (X[0] - X[1]).abs() if isinstance(X, (list, tuple)) else X
        u = torch.as_tensor(np.asarray(utility.cpu() if hasattr(utility, "cpu") else utility, np.float32)).to(rows.device)
        query_idx = diverse_minibatch_device(rows, u, k, beta=beta, iters=iters, seed=random_state)[0].cpu().numpy().astype(np.int64)
    else:
        rows = _rows(X)
        u = np.asarray(utility, np.float32)
        if u.shape != (len(rows),):
            raise ValueError("the classifier's uncertainty has shape %s for %d rows" % (u.shape, len(rows)))
        k = min(k, len(rows))
        m = min(len(rows), int(beta) * k)
        top = np.argsort(-u, kind="stable")[:m]                       # the m largest, ties to the lower index
        near = _host_pick(rows[top], k, iters, random_state, weights=u[top])
        query_idx = np.where(near >= 0, top[np.clip(near, 0, None)], -1).astype(np.int64)
    query_idx = query_idx[query_idx >= 0]
    return query_idx, _instances(X, query_idx, on_device)
