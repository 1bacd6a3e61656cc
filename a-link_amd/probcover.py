"""probcover — the fixed-radius neighbour graph of a pool, its purity radius and ProbCover queries (Yehuda, Dekel, Hacohen &
Weinshall 2022, "Active Learning Through a Covering Lens").  EXTENSION: the reference imports its strategies
from modAL, which has no such sampler; no reference driver names these.

TypiClust's successor for the low-budget regime, from the same authors: put a ball of radius delta round every pool row, and
query, one after another, the row whose ball covers the most rows no earlier ball covers — greedy maximum coverage.  delta is
the largest radius at which balls stay pure with respect to a clustering of the pool.

The rule (include/alink_hip.h, alink_ball_count, states it in full):

    eligible    a row whose group (`groups`, None: one group) is >= 0 and whose squared norm is finite in float32.  Any other row
                has no ball, lies in nobody's ball, is never covered and is never picked.
    radius      radius2 = float32(delta * delta): the radius enters every comparison as that float32
    edge        j is in ball(n) when both are eligible and t(n, j) = |x_n|^2 + |x_j|^2 - 2 x_n . x_j < radius2 — strict, as in the
                paper's code — or j == n.  Symmetric: n covers j exactly when j covers n.  Groups do not limit a ball.
    purity      t_other(n) = the least t(n, j) over eligible j of another group (ties to the lower j; +inf and j = -1 where there is
                none): the ball of radius2 r2 round n is impure exactly when t_other(n) < r2.  With M eligible rows and
                m = floor((1 - alpha) M), the purity radius has radius2 = the (m + 1)-th smallest t_other: the largest at which at
                most m balls are impure — attained, because the edge test is strict.
    graph       CSR: offsets int64 (N + 1), nbr int32 (E), a row's neighbours ascending
    greedy      seeds (the labelled rows) have their balls covered first.  Then per pick: degree(u) = the rows of ball(u) not yet
                covered; the pick is the u of largest degree by `>` from 0, ties to the lower u; its ball is covered; gain = its
                degree.  Once the largest degree is 0 the pool is covered: that pick and every later one is -1 with gain 0.

`ball_graph`, `nearest_other`, `purity_radius`, `max_coverage` and `probcover` are that rule in host float64 NumPy (an N x N matrix:
small pools only); the `_device` forms are alink_ball_count, alink_ball_fill and alink_max_coverage (probcover.hip: the N x N scores
on the matrix cores, never in memory; a streaming recount per pick).  On the device t is formed in float32 in an order that makes
t(n, j) and t(j, n) the same bits; where nothing rounds, as on small-integer rows, host and device agree bit for bit.

Not built: distances stored with the edges, skipping tiles by a spatial bound, an incremental-degree greedy, a cosine metric,
balls round a separate set of centres (cal.knn_rect_device searches a separate set, for lists of k, not for balls), several
ranks' pools in one call.
"""
import numpy as np

from . import badge as _badge
from . import cluster as _cluster
from .batch import _rows
from .typiclust import _groups_host, _labelled_indices


def radius2_of(delta):
    """float32(delta * delta), the number every edge test compares with; ValueError unless it is finite and > 0"""
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = np.float32(np.float64(delta) * np.float64(delta))
    if not (np.float64(delta) > 0 and np.isfinite(r2) and r2 > 0):
        raise ValueError("delta = %r: it must be > 0 and its square finite and > 0 in float32" % (delta,))
    return r2


def _host_rows(rows):
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    return X


def _t_matrix(X, groups):
    """-> (t float64 (N, N), eligible bool (N,), groups int64 (N,))"""
    g = _groups_host(groups, len(X))
    with np.errstate(invalid="ignore", over="ignore"):
        norms = (X * X).sum(axis=1)
        alive = (g >= 0) & np.isfinite(norms.astype(np.float32))
        Xa = np.where(alive[:, None], X, 0.0)
        na = np.where(alive, norms, 0.0)
        t = (na[:, None] + na[None, :]) - 2.0 * (Xa @ Xa.T)
    return t, alive, g


def ball_graph(rows, delta, groups=None):
    """The delta-ball graph of the (N, D) array `rows` on the host, the rule of the module docstring in float64.  EXTENSION.
    -> (offsets int64 (N + 1,), nbr int32 (E,)): CSR, a row's neighbours in ascending order, itself among them."""
    X = _host_rows(rows)
    r2 = np.float64(radius2_of(delta))
    t, alive, _ = _t_matrix(X, groups)
    edge = ((t < r2) | np.eye(len(X), dtype=bool)) & alive[:, None] & alive[None, :]
    offsets = np.zeros(len(X) + 1, np.int64)
    offsets[1:] = np.cumsum(edge.sum(axis=1))
    return offsets, np.nonzero(edge)[1].astype(np.int32)                   # (row-major: ascending within a row)


def nearest_other(rows, groups):
    """Per row the nearest eligible row of ANOTHER group, on the host.  EXTENSION.
    -> (t_other float64 (N,), j_other int32 (N,)): the least t by `<` from +inf, ties to the lower j; +inf and -1 where none."""
    X = _host_rows(rows)
    if groups is None:
        raise ValueError("groups: purity is measured against a grouping")
    t, alive, g = _t_matrix(X, groups)
    ok = alive[:, None] & alive[None, :] & (g[:, None] != g[None, :]) & (t < np.inf)
    t = np.where(ok, t, np.inf)
    j = np.argmin(t, axis=1)                                               # the first of equal minima
    t_other = t[np.arange(len(X)), j]
    return t_other, np.where(t_other < np.inf, j, -1).astype(np.int32)


def _rank(M, alpha):
    """m = floor((1 - alpha) M) for M eligible rows: the purity radius is the (m + 1)-th smallest t_other"""
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha = %r outside 0 .. 1" % (alpha,))
    if M < 1:
        raise ValueError("purity_radius: no eligible row")
    return min(int(np.floor((1.0 - float(alpha)) * M)), M - 1)


def _delta_of(v):
    """the delta whose radius2_of is the largest float32 <= v; ValueError for +inf (no ball is ever impure) and for v <= 0"""
    if not v < np.inf:
        raise ValueError("purity_radius: fewer balls can turn impure than alpha allows — every radius is pure enough (radius +inf)")
    r2 = np.float32(v)
    if np.float64(r2) > v:
        r2 = np.nextafter(r2, np.float32(-np.inf))
    if not r2 > 0:
        raise ValueError("purity_radius: rows of different groups coincide — no radius > 0 is pure enough")
    delta = float(np.sqrt(np.float64(r2)))
    assert radius2_of(delta) == r2
    return delta


def purity_radius(rows, groups, alpha=0.95):
    """The largest delta at which at least alpha of the eligible rows have a pure ball, on the host.  EXTENSION.  radius2 = the
    (m + 1)-th smallest t_other, m = floor((1 - alpha) M), rounded DOWN to float32 (radius2_of(delta) is that float32 exactly).
    ValueError when that value is +inf (fewer than m + 1 rows have a row of another group at all) or not > 0."""
    t_other, _ = nearest_other(rows, groups)
    _, alive, _ = _t_matrix(_host_rows(rows), groups)
    M = int(alive.sum())
    m = _rank(M, alpha)
    return _delta_of(float(np.sort(t_other[alive])[m]))


def _check_graph(offsets, nbr):
    offsets, nbr = np.asarray(offsets, np.int64), np.asarray(nbr, np.int64)
    if offsets.ndim != 1 or len(offsets) < 2 or offsets[0] != 0 or (np.diff(offsets) < 0).any() or offsets[-1] != len(nbr):
        raise ValueError("offsets: N + 1 ascending values from 0 to len(nbr) are needed")
    N = len(offsets) - 1
    if len(nbr) and (nbr.min() < 0 or nbr.max() >= N):
        raise ValueError("nbr: a row index outside 0 .. %d" % (N - 1))
    return offsets, nbr, N


def _check_k(k):
    if int(k) != k or int(k) < 1:
        raise ValueError("k = %r must be an integer >= 1" % (k,))
    return int(k)


def max_coverage(offsets, nbr, k, seeds=(), covered=None):
    """Greedy maximum coverage over a CSR graph on the host, the `greedy` rule of the module docstring.  EXTENSION.
    seeds: rows whose balls are covered before the first pick; covered: None or N flags of rows covered already (not changed).
    -> (picks int32 (k,), gain int32 (k,), covered uint8 (N,))."""
    offsets, nbr, N = _check_graph(offsets, nbr)
    k = _check_k(k)
    cov = np.zeros(N, bool) if covered is None else np.array(covered).astype(bool).reshape(-1)
    if cov.shape != (N,):
        raise ValueError("covered: %d flags are needed" % N)
    for s in _labelled_indices(seeds, N):
        cov[nbr[offsets[s]:offsets[s + 1]]] = True
    picks, gain = np.full(k, -1, np.int32), np.zeros(k, np.int32)
    for t in range(k):
        run = np.concatenate([[0], np.cumsum(~cov[nbr])])
        degree = run[offsets[1:]] - run[offsets[:-1]]
        u = int(np.argmax(degree))                                         # the first of equal maxima: ties to the lower row
        if degree[u] <= 0:
            break
        picks[t], gain[t] = u, degree[u]
        cov[nbr[offsets[u]:offsets[u + 1]]] = True
    return picks, gain, cov.astype(np.uint8)


def _plan(N, labelled, n_instances, fill):
    n = _cluster._check_instances(n_instances)
    lab = _labelled_indices(labelled, N)
    if N - len(lab) < n:
        raise ValueError("n_instances = %d but only %d of the %d rows are not labelled" % (n, N - len(lab), N))
    if fill not in (None, "random"):
        raise ValueError("fill = %r: None or 'random'" % (fill,))
    return lab, n


def _finish(picks, gain, covered, eligible, lab, n, fill, random_state, delta, edges):
    """the picks before exhaustion, the random fill and the info dict, the same on both routes (host arrays)"""
    real = picks[picks >= 0].astype(np.int64)
    exhausted = len(real) < n
    out = real
    if exhausted and fill == "random":
        free = eligible.copy()
        free[lab] = False
        free[real] = False
        cand = np.flatnonzero(free)
        take = min(n - len(real), len(cand))
        if take:
            out = np.concatenate([real, np.random.RandomState(random_state).choice(cand, take, replace=False).astype(np.int64)])
    M = int(eligible.sum())
    info = {"delta": float(delta), "edges": int(edges), "covered": float(covered[eligible].sum()) / M if M else 0.0,
            "gain": gain[:len(real)].astype(np.int64), "exhausted": bool(exhausted)}
    return out, info


def probcover(rows, labelled, n_instances, delta=None, groups=None, alpha=0.95, fill=None, random_state=None):
    """ProbCover on the host: n_instances queries among the rows of the (N, D) array `rows`, everything in float64 NumPy.  EXTENSION.

    labelled   row indices into `rows`: their balls are covered before the first pick, so they are never picked
    delta      the radius; None: purity_radius(rows, groups, alpha)
    groups     None, or N integers: rows of group < 0 are not eligible; with delta=None the clustering purity is measured against
    fill       None: fewer than n_instances picks once the pool is covered; "random": the rest drawn uniformly, without
               replacement, from the eligible rows neither labelled nor picked (np.random.RandomState(random_state))
    -> (picks int64, info): info holds "delta", "edges" (E), "covered" (the share of eligible rows covered after the greedy picks),
    "gain" (per greedy pick) and "exhausted" (the pool was covered before n_instances picks)."""
    X = _host_rows(rows)
    lab, n = _plan(len(X), labelled, n_instances, fill)
    if delta is None:
        delta = purity_radius(X, groups, alpha)
    offsets, nbr = ball_graph(X, delta, groups)
    picks, gain, covered = max_coverage(offsets, nbr, n, seeds=lab)
    eligible = np.diff(offsets) > 0
    return _finish(picks, gain, covered, eligible, lab, n, fill, random_state, delta, len(nbr))


# ---- device forms -------------------------------------------------------------------------------------------------------------
def _pool(rows, groups, what):
    import torch
    from .batch import _pool_rows
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if N < 1:
        raise ValueError("%s: the pool is empty" % what)
    if D > _cluster.MAX_D:
        raise ValueError("rows have D = %d columns, beyond the %d a device row may have" % (D, _cluster.MAX_D))
    if groups is not None:
        if not isinstance(groups, torch.Tensor) or groups.device != dev or groups.dtype is not torch.int32 or groups.shape != (N,):
            raise ValueError("groups: an int32 tensor of %d values on the pool's device is needed" % N)
        groups = groups.contiguous()
    return (left, right, li, ri), N, D, dev, groups


def _ball_count(pool, radius2, want_deg, want_other):
    """alink_ball_count on _pool's result -> (deg or None, t_other or None, j_other or None) on the device"""
    import torch
    from . import _abi, net_host
    (left, right, li, ri), N, D, dev, groups = pool
    if want_other and groups is None:
        raise ValueError("groups: purity is measured against a grouping")
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_ball_scratch_bytes(N, D), dev)
    deg = torch.empty(N, dtype=torch.int32, device=dev) if want_deg else None
    t_other = torch.empty(N, dtype=torch.float32, device=dev) if want_other else None
    j_other = torch.empty(N, dtype=torch.int32, device=dev) if want_other else None
    _abi.check(lib.alink_ball_count(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(groups), float(radius2),
                                    _abi.ptr(deg), _abi.ptr(t_other), _abi.ptr(j_other), sp, _abi.current_stream(dev)), "alink_ball_count")
    return deg, t_other, j_other


def ball_count_device(rows, delta, groups=None):
    """The size of every row's delta-ball on the GPU (alink_ball_count): rows, groups as in ball_graph_device.  EXTENSION.
    -> int32 (N,) on the device, 0 for a row that is not eligible.  Nothing is synchronised or read back."""
    return _ball_count(_pool(rows, groups, "ball_count_device"), radius2_of(delta), True, False)[0]


def ball_graph_device(rows, delta, groups=None):
    """The delta-ball graph of a pool on the GPU: alink_ball_count, torch.cumsum in int64, ONE read-back of E to allocate,
    alink_ball_fill.  EXTENSION.

    rows    the pool as in cluster.kmeans_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri)
    groups  None, or CUDA int32 (N,): rows of group < 0 are not eligible
    -> (offsets int64 (N + 1,), nbr int32 (E,)) on the device.  The fill's mismatch count is read back and asserted to be 0."""
    import torch
    from . import _abi, net_host
    r2 = radius2_of(delta)
    pool = _pool(rows, groups, "ball_graph_device")
    (left, right, li, ri), N, D, dev, groups = pool
    deg = _ball_count(pool, r2, True, False)[0]
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(deg, 0, dtype=torch.int64)
    E = int(offsets[-1])
    nbr = torch.empty(E, dtype=torch.int32, device=dev)
    if E == 0:
        return offsets, nbr
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_ball_scratch_bytes(N, D), dev)
    mismatch = torch.empty(1, dtype=torch.int32, device=dev)
    _abi.check(lib.alink_ball_fill(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(groups), float(r2),
                                   _abi.ptr(offsets), E, _abi.ptr(nbr), _abi.ptr(mismatch), sp, _abi.current_stream(dev)),
               "alink_ball_fill")
    bad = int(mismatch)
    assert bad == 0, "alink_ball_fill: %d rows' balls did not fill their spans" % bad
    return offsets, nbr


def nearest_other_device(rows, groups):
    """Per row the nearest eligible row of another group on the GPU (alink_ball_count's purity outputs).  EXTENSION.
    -> (t_other float32 (N,), j_other int32 (N,)) on the device.  Nothing is synchronised or read back."""
    return _ball_count(_pool(rows, groups, "nearest_other_device"), 1.0, False, True)[1:]


def purity_radius_device(rows, groups, alpha=0.95):
    """purity_radius on the GPU: ONE alink_ball_count pass (degrees > 0 name the eligible rows), then torch.sort.  EXTENSION.
    Reads back two numbers.  -> delta (float)."""
    import torch
    deg, t_other, _ = _ball_count(_pool(rows, groups, "purity_radius_device"), 1.0, True, True)
    M = int((deg > 0).sum())
    m = _rank(M, alpha)
    # (a row that is not eligible holds +inf: behind every finite value, like an eligible row without a row of another group)
    return _delta_of(float(torch.sort(t_other).values[m]))


def max_coverage_device(offsets, nbr, k, seeds=None, covered=None):
    """Greedy maximum coverage over a CSR graph on the GPU (alink_max_coverage).  EXTENSION.

    offsets  CUDA int64 (N + 1,); nbr: CUDA int32 (E,) — ball_graph_device's
    seeds    None, or row indices (host integers or a CUDA int32 tensor) whose balls are covered before the first pick
    covered  None, or CUDA uint8 (N,): rows covered already (copied)
    -> (picks int32 (k,), gain int32 (k,), covered uint8 (N,)) on the device.  Nothing is synchronised or read back."""
    import torch
    from . import _abi, net_host
    if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.dtype is not torch.int64 or offsets.dim() != 1 or offsets.numel() < 2:
        raise ValueError("offsets: a CUDA int64 tensor of N + 1 values is needed")
    dev, N = offsets.device, offsets.numel() - 1
    if not isinstance(nbr, torch.Tensor) or nbr.device != dev or nbr.dtype is not torch.int32 or nbr.dim() != 1:
        raise ValueError("nbr: a 1-D int32 tensor on the offsets' device is needed")
    k = _check_k(k)
    offsets, nbr = offsets.contiguous(), nbr.contiguous()
    if nbr.numel() == 0:
        nbr = torch.zeros(1, dtype=torch.int32, device=dev)                # (a graph without edges: nothing is read through it)
    if seeds is not None and not isinstance(seeds, torch.Tensor):
        seeds = torch.from_numpy(_labelled_indices(seeds, N).astype(np.int32)).to(dev)
    if seeds is not None:
        if seeds.device != dev or seeds.dtype is not torch.int32 or seeds.dim() != 1:
            raise ValueError("seeds: a 1-D int32 tensor on the offsets' device is needed")
        seeds = seeds.contiguous() if seeds.numel() else None
    if covered is None:
        cov = torch.zeros(N, dtype=torch.uint8, device=dev)
    else:
        if not isinstance(covered, torch.Tensor) or covered.device != dev or covered.dtype is not torch.uint8 or covered.shape != (N,):
            raise ValueError("covered: a uint8 tensor of %d flags on the offsets' device is needed" % N)
        cov = covered.clone().contiguous()
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_max_coverage_scratch_bytes(N, k), dev)
    picks = torch.empty(k, dtype=torch.int32, device=dev)
    gain = torch.empty(k, dtype=torch.int32, device=dev)
    _abi.check(lib.alink_max_coverage(_abi.ptr(offsets), _abi.ptr(nbr), N, _abi.ptr(seeds), 0 if seeds is None else seeds.numel(), k,
                                      _abi.ptr(cov), _abi.ptr(picks), _abi.ptr(gain), sp, _abi.current_stream(dev)), "alink_max_coverage")
    return picks, gain, cov


def probcover_device(rows, labelled, n_instances, delta=None, groups=None, alpha=0.95, fill=None, random_state=None):
    """ProbCover on the GPU: purity_radius_device (with delta=None), ball_graph_device, max_coverage_device.  EXTENSION.

    rows      the pool as in ball_graph_device; labelled: host integers, row indices into it
    groups    None, or CUDA int32 (N,) — cluster.kmeans_device's "assign": eligibility, and with delta=None the purity's grouping
    the rest as in probcover.  -> (picks int64 NumPy array, info), probcover's; info["offsets"], info["nbr"] and
    info["covered_rows"] (uint8 (N,)) are the device tensors.  Read back: E, the fill's mismatch count, with delta=None the
    radius, and at the end picks, gains and the N-byte covered and eligible flags."""
    import torch
    from .batch import _pool_rows
    N, dev = _pool_rows(rows, torch)[4::2]
    if N < 1:
        raise ValueError("probcover_device: the pool is empty")
    lab, n = _plan(N, labelled, n_instances, fill)
    if delta is None:
        delta = purity_radius_device(rows, groups, alpha)
    offsets, nbr = ball_graph_device(rows, delta, groups)
    picks, gain, covered = max_coverage_device(offsets, nbr, n, seeds=lab if len(lab) else None)
    eligible = (offsets[1:] > offsets[:-1]).cpu().numpy()
    out, info = _finish(picks.cpu().numpy(), gain.cpu().numpy(), covered.cpu().numpy(), eligible, lab, n, fill, random_state, delta,
                        nbr.numel())
    info["offsets"], info["nbr"], info["covered_rows"] = offsets, nbr, covered
    return out, info


def _n_clusters(n_clusters, labelled, n, max_clusters=500):
    if n_clusters is None:
        return max(2, min(labelled + n, max_clusters, _cluster.MAX_K))     # TypiClust's rule: one cluster per labelled row and query
    if int(n_clusters) != n_clusters or int(n_clusters) < 2:
        raise ValueError("n_clusters = %r must be an integer >= 2" % (n_clusters,))
    return int(n_clusters)


def probcover_sampling(classifier, X, n_instances=1, delta=None, n_clusters=None, alpha=0.95, iters=10, random_state=None):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=probcover_sampling)): ProbCover queries among the rows of X, an
    (N, D) array or pair input [left, right] (rows |left - right|).  EXTENSION.  The learner's labelled rows
    (`classifier.X_training`, as typiclust.typiclust_sampling takes them; None: none) are appended behind the pool and named as
    `labelled`; the scorer itself is not consulted.  delta=None: the purity radius (alpha) against a k-means clustering of pool and
    labelled rows into n_clusters groups (None: min(labelled + n_instances, 500)) from k-means++ seeds, `iters` updates.
    fill="random": a call always returns n_instances rows.  CUDA tensors go through probcover_device, anything else through
    probcover.  random_state: the seed of the k-means++ uniforms and of the fill.  -> (query_idx, instances): the instances as the
    other samplers of this package return them for pair input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    training = getattr(classifier, "X_training", None)
    on_device = _cluster._is_cuda(X)
    n = _cluster._check_instances(n_instances)
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
        groups = None
        if delta is None:
            K = _n_clusters(n_clusters, rows.shape[0] - N, n)
            groups = _cluster.kmeans_device(rows, K, iters=iters, seed=random_state)["assign"]
        query_idx, _ = probcover_device(rows, np.arange(N, rows.shape[0]), n, delta=delta, groups=groups, alpha=alpha, fill="random",
                                        random_state=random_state)
    else:
        rows = _rows(X)
        N = len(rows)
        if training is not None:
            rows = np.vstack([rows, _rows(training)])
        groups = None
        if delta is None:
            K = _n_clusters(n_clusters, len(rows) - N, n)
            seeds, _ = _badge.kmeans_pp(rows, K, np.random.RandomState(random_state).random_sample(K))
            centres = np.full((K, rows.shape[1]), np.inf, np.float32)
            centres[seeds >= 0] = rows[seeds[seeds >= 0]]
            groups = _cluster.kmeans(rows, centres, iters)["assign"]
        query_idx, _ = probcover(rows, np.arange(N, len(rows)), n, delta=delta, groups=groups, alpha=alpha, fill="random",
                                 random_state=random_state)
    return query_idx, _cluster._instances(X, query_idx, on_device)
