"""badge — BADGE batches (Ash et al. 2020, "Deep batch active learning by diverse, uncertain gradient lower bounds"): k-means++
seeding (Arthur & Vassilvitskii 2007) over the last layer's gradient embeddings of the pair scorer.  EXTENSION (DESIGN.md §0,
X10): the reference imports its strategies from modAL, which has no such sampler; no reference driver names this one.

egl.py writes, for every pair, the last layer's weight gradient under the label the scorer itself would give.  Its length says
how much the pair would move the scorer, its direction in which way.  A BADGE batch is k-means++ seeding over those rows: the
first centre is the row of largest norm, every later centre is DRAWN with probability proportional to its squared distance to
the nearest centre so far.  Large gradients are favoured, a burst of near-duplicate pairs gets one pick (a duplicate of a
centre has distance 0 and cannot be drawn), and there is no weight to set by hand, as batch.py's alpha is.

This is the package's only sampling strategy, so the draw is pinned (include/alink_hip.h, alink_kmeanspp, states it in full):

    pick 0   `first`, or the first row of largest squared norm; potential[0] = NaN
    d2_n     = min over the picks so far of |x_n - x_p|^2
    w_n      = d2_n where 0 < d2_n < inf, else 0            C_n = w_0 + ... + w_n,  T = C_(N-1)
    pick t   = the smallest n with C_n > uniforms[t] * T (none, the product rounded up to T: the last row with w > 0)
    potential[t] = T; once T is 0 (fewer distinct rows than picks) this and every later pick is -1 with potential 0

uniforms[0] is never read, so a stream of uniforms means the same with and without `first`.  `kmeans_pp` is host float64 NumPy
(np.cumsum / np.searchsorted); `kmeans_pp_device` is the same rule for rows resident on the GPU (alink_kmeanspp, kmeanspp.hip:
one streaming pass per pick, d2 in float32 in batch.py's summation order, the sums in float64) — where no sum rounds, as on
small-integer rows, the two give the same picks and potentials bit for bit.  `badge_device` feeds it
egl.expected_gradient_length_device's embeddings, `badge_sampling` is modAL-shaped.  Not built: several ranks' pools in one call,
labelled rows as centres that exist before the first pick, a bf16-mode head, fusing the embedding into the distance pass.
"""
import numpy as np

from . import egl as _egl

MAX_D = 8192                                               # columns of a device row: the picked row is held in LDS (RB_MAX_D, batch_rows.h)


def _uniforms(uniforms, seed, k):
    """the k float64 uniforms of a call, checked -> a contiguous float64 array of exactly k"""
    if uniforms is None:
        return np.random.RandomState(seed).random_sample(k)
    u = np.ascontiguousarray(np.asarray(uniforms, np.float64).reshape(-1))
    if u.size < k:
        raise ValueError("uniforms: %d values for %d picks (one per pick; entry 0 is never read)" % (u.size, k))
    u = u[:k]
    if not ((u >= 0.0) & (u < 1.0)).all():
        raise ValueError("uniforms: every value must lie in [0, 1)")
    return u


def kmeans_pp(rows, n_instances, uniforms, first=None):
    """k-means++ seeding of the (N, D) array `rows` on the host, the rule of the module docstring in float64.  EXTENSION.

    n_instances  picks, clipped to N
    uniforms     at least that many float64 values in [0, 1); entry 0 is never read
    first        None: pick 0 is the first row of largest squared norm (a NaN norm never wins); else that row index
    -> (idx int64 (k,), potential float64 (k,)); -1 / 0 once fewer distinct rows than picks are left."""
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    N = X.shape[0]
    if int(n_instances) < 1:
        raise ValueError("n_instances = %r must be at least 1" % (n_instances,))
    k = min(int(n_instances), N)
    u = _uniforms(uniforms, None, k)
    idx, potential = np.full(k, -1, np.int64), np.zeros(k, np.float64)
    potential[0] = np.nan
    with np.errstate(invalid="ignore", over="ignore"):
        if first is None:
            norms = (X * X).sum(axis=1)
            if np.isnan(norms).all():
                return idx, potential
            p = int(np.argmax(np.where(np.isnan(norms), -np.inf, norms)))
        else:
            p = int(first)
            if not 0 <= p < N:
                raise ValueError("first = %r outside 0 .. %d" % (first, N - 1))
        idx[0] = p
        d2 = ((X - X[p]) ** 2).sum(axis=1)
        for t in range(1, k):
            w = np.where((d2 > 0) & (d2 < np.inf), d2, 0.0)
            C = np.cumsum(w)
            T = C[-1]
            if not T > 0:
                break
            n = int(np.searchsorted(C, u[t] * T, side="right"))    # the first n with C_n > target
            if n >= N:
                n = int(np.flatnonzero(w > 0)[-1])
            idx[t], potential[t] = n, T
            d2 = np.fmin(d2, ((X - X[n]) ** 2).sum(axis=1))
    return idx, potential


def kmeans_pp_device(rows, n_instances, uniforms=None, seed=None, first=None):
    """k-means++ seeding of a pool on the GPU (alink_kmeanspp).  EXTENSION.

    rows         the pool as in batch.ranked_batch_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri) —
                 row n is |left[li[n]] - right[ri[n]]|, formed on the fly, never materialised
    n_instances  picks, clipped to N
    uniforms     float64 array of at least k values in [0, 1) (entry 0 is never read); None: np.random.RandomState(seed).random_sample(k)
    first        None: pick 0 is the row of largest squared norm; else that row index
    -> (idx int32 (k,), potential float64 (k,)) on the device: the picks in order (-1 once fewer distinct rows than picks are
    left) and the k-means potential each was drawn from (potential[0] is NaN).  Nothing is synchronised or read back except, in
    the pair form, the range check of li / ri."""
    import torch
    from . import _abi, net_host
    from .batch import _pool_rows
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if int(n_instances) < 1:
        raise ValueError("n_instances = %r must be at least 1" % (n_instances,))
    if N < 1:
        raise ValueError("kmeans_pp_device: the pool is empty")
    if first is not None and not 0 <= int(first) < N:
        raise ValueError("first = %r outside 0 .. %d" % (first, N - 1))
    k = min(int(n_instances), N)
    # the k uniforms go up from pinned memory on the current stream: a pageable copy would make the host wait for the stream
    u = torch.from_numpy(_uniforms(uniforms, seed, k)).pin_memory().to(dev, non_blocking=True)
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_kmeanspp_scratch_bytes(N, k), dev)
    idx = torch.empty(k, dtype=torch.int32, device=dev)
    potential = torch.empty(k, dtype=torch.float64, device=dev)
    _abi.check(lib.alink_kmeanspp(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(u),
                                  -1 if first is None else int(first), k, _abi.ptr(idx), _abi.ptr(potential), sp,
                                  _abi.current_stream(dev)), "alink_kmeanspp")
    return idx, potential


def badge_device(head, L, R, li=None, ri=None, n_instances=1, uniforms=None, seed=None):
    """A BADGE batch of the pairs (L[n], R[n]) or (L[li[n]], R[ri[n]]) on the GPU: egl.expected_gradient_length_device's gradient
    embeddings (want=("emb",)), then kmeans_pp_device over them.  EXTENSION.  head: a DenseHead in the float32 compute mode.
    -> (idx int32 (k,), potential float64 (k,)) on the device, indices into the pairs."""
    emb = _egl.expected_gradient_length_device(head, L, R, li, ri, want=("emb",))["emb"]
    return kmeans_pp_device(emb, n_instances, uniforms=uniforms, seed=seed)


def badge_sampling(classifier, X, n_instances=1, random_state=None):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=badge_sampling)): a BADGE batch of n_instances pairs of
    X = [left, right].  EXTENSION.  `classifier`: a DenseHead, or a learner / estimator that exposes siamese_net.get_weights().
    CUDA tensors go through the device route (the head must be a DenseHead: there is no fallback), anything else through
    egl.gradient_embedding and kmeans_pp.  random_state: the seed of np.random.RandomState for the uniforms — the same seed gives
    the same picks.  -> (query_idx, instances): the picks in order, without the -1 of an exhausted pool; the instances as the
    other samplers of this package return them for pair input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    net = _egl._head_of(classifier)
    on_device = hasattr(X[0], "is_cuda") and X[0].is_cuda
    if on_device:
        if not hasattr(net, "badge_device"):
            raise TypeError("badge_sampling on CUDA tensors needs a DenseHead (got %s)" % type(net).__name__)
        query_idx = net.badge_device(X[0], X[1], n_instances=n_instances, seed=random_state)[0].cpu().numpy().astype(np.int64)
    else:
        emb = _egl.gradient_embedding(net.get_weights(), X)
        k = min(int(n_instances), len(emb))
        query_idx, _ = kmeans_pp(emb, k, np.random.RandomState(random_state).random_sample(k))
    query_idx = query_idx[query_idx >= 0]
    if on_device:
        import torch
        take = torch.from_numpy(query_idx).to(X[0].device)
        return query_idx, [X[0][take], X[0][take]]
    return query_idx, [X[0][query_idx], X[0][query_idx]]
