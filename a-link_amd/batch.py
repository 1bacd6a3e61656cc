"""batch — ranked batch-mode sampling of modAL.batch (Cardoso et al. 2017), patched for pair input like uncertainty.py and
disagreement.py.  EXTENSION: the reference imports its strategies from modAL; no reference driver names
this one.

Top-k samplers spend a batch on near-duplicates: every frame of one burst scores alike.  Here each pick weighs a row's
utility against its distance to everything labelled or already picked.  With N pool rows, M labelled rows, utilities u:

    d_n     = min over the labelled rows and the picks so far of dist(x_n, .)
    alpha_t = (N - t) / (N + M)                       |unlabelled| / (|unlabelled| + |labelled|), picks count as labelled
    score_n = alpha_t (1 - 1 / (1 + d_n)) + (1 - alpha_t) u_n         over the rows not yet picked
    pick_t  = argmax score (np.argmax: the first maximum)

`select_cold_start_instance`, `select_instance`, `ranked_batch` and `uncertainty_batch_sampling` have modAL's signatures and
are host float64 NumPy + sklearn's pairwise_distances_argmin_min, one full call per pick, any sklearn metric.  Without
labelled rows the first pick is the row with the least mean distance to all rows (modAL's cold start); it is masked like
every other pick.  `ranked_batch_device` is the same rule with the Euclidean metric for a pool resident on the GPU
(alink_ranked_batch, batch.hip: one streaming pass per pick); it needs a labelled row.  `ranked_batch_cold_device` is the
form without one: the cold start's row comes from density.information_density_device (alink_information_density,
density.hip: every pool row against every other, the host form's N x N float64 matrix never built) and becomes the one
labelled row of ranked_batch_device over the rest of the pool.

A pair input X = [left, right] is represented by the rows |left - right|, which is what the pair scorer itself sees
(code/siamese.py:27-35); the learner's X_training likewise.
Kept quirk: for pair input the sampler returns `[X[0][idx], X[0][idx]]` — the LEFT array twice (code/uncertainty.py:159,187,217).
"""
import numpy as np

from .uncertainty import classifier_uncertainty


def _rows(X):
    """array -> itself in float64; pair input [left, right] -> |left - right|"""
    if isinstance(X, (list, tuple)):
        return np.abs(np.asarray(X[0], np.float64) - np.asarray(X[1], np.float64))
    return np.asarray(X, np.float64)


def select_cold_start_instance(X, metric, n_jobs):
    """modAL.batch.select_cold_start_instance: (index, row as (1, D)) of the row with the least mean distance to all rows."""
    from sklearn.metrics.pairwise import pairwise_distances
    n_jobs = n_jobs if n_jobs else 1
    average_distances = np.mean(pairwise_distances(X, metric=metric, n_jobs=n_jobs), axis=0)
    best = int(np.argmin(average_distances))
    return best, X[best].reshape(1, -1)


def select_instance(X_training, X_pool, X_uncertainty, mask, metric, n_jobs):
    """modAL.batch.select_instance: one pick among the rows `mask` leaves -> (index in X_pool, row as (1, D), mask with it cleared)."""
    from sklearn.metrics.pairwise import pairwise_distances, pairwise_distances_argmin_min
    X_pool_masked = X_pool[mask]
    n_labeled, n_unlabeled = X_training.shape[0], X_pool_masked.shape[0]
    alpha = n_unlabeled / (n_unlabeled + n_labeled)
    if n_jobs == 1 or n_jobs is None:
        _, distance_scores = pairwise_distances_argmin_min(X_pool_masked.reshape(n_unlabeled, -1), X_training.reshape(n_labeled, -1),
                                                           metric=metric)
    else:
        distance_scores = pairwise_distances(X_pool_masked.reshape(n_unlabeled, -1), X_training.reshape(n_labeled, -1), metric=metric,
                                             n_jobs=n_jobs).min(axis=1)
    similarity_scores = 1 / (1 + distance_scores)
    scores = alpha * (1 - similarity_scores) + (1 - alpha) * X_uncertainty[mask]
    best = int(np.flatnonzero(mask)[np.argmax(scores)])
    mask[best] = False
    return best, np.expand_dims(X_pool[best], axis=0), mask


def ranked_batch(classifier, unlabeled, uncertainty_scores, n_instances, metric, n_jobs):
    """modAL.batch.ranked_batch: the indices of min(n_instances, N) picks, in pick order.  `classifier.X_training` (array, pair
    list or None) is the labelled set; `unlabeled` an (N, D) array or a pair list."""
    unlabeled = _rows(unlabeled)
    uncertainty_scores = np.asarray(uncertainty_scores, np.float64)
    mask = np.ones(unlabeled.shape[0], bool)
    if classifier.X_training is None:
        best, labeled = select_cold_start_instance(X=unlabeled, metric=metric, n_jobs=n_jobs)
        mask[best] = False
        ranking = [best]
    else:
        labeled = _rows(classifier.X_training)
        ranking = []
    ceiling = min(unlabeled.shape[0], n_instances) - len(ranking)
    for _ in range(ceiling):
        index, instance, mask = select_instance(X_training=labeled, X_pool=unlabeled, X_uncertainty=uncertainty_scores, mask=mask,
                                                metric=metric, n_jobs=n_jobs)
        labeled = np.vstack((labeled, instance))
        ranking.append(index)
    return np.array(ranking, dtype=np.int64)


def uncertainty_batch_sampling(classifier, X, n_instances=20, metric='euclidean', n_jobs=None, **uncertainty_measure_kwargs):
    """modAL.batch.uncertainty_batch_sampling: ranked batch with classification uncertainty (1 - max probability) as utility."""
    uncertainty = classifier_uncertainty(classifier, X, **uncertainty_measure_kwargs)
    query_idx = ranked_batch(classifier, unlabeled=X, uncertainty_scores=uncertainty, n_instances=n_instances, metric=metric,
                             n_jobs=n_jobs)
    if isinstance(X, (list, tuple)):
        return query_idx, [X[0][query_idx], X[0][query_idx]]
    return query_idx, X[query_idx]


# ---- device form: init + one streaming pass per pick, everything resident ---------------------------------------------------
def _f32_matrix(name, t, torch, device=None, cols=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s: a CUDA tensor is needed (got %s)" % (name, "a CPU tensor" if isinstance(t, torch.Tensor) else type(t).__name__))
    if t.dtype is not torch.float32:
        raise ValueError("%s: float32 is needed (got %s)" % (name, t.dtype))
    if t.dim() != 2:
        raise ValueError("%s: a 2-D (rows, D) tensor is needed (got shape %s)" % (name, tuple(t.shape)))
    if device is not None and t.device != device:
        raise ValueError("%s is on %s, the pool on %s" % (name, t.device, device))
    if cols is not None and t.shape[1] != cols:
        raise ValueError("%s has D = %d, the pool D = %d" % (name, t.shape[1], cols))
    return t.contiguous()


def _pool_rows(rows, torch):
    """the pool argument of the device forms, checked -> (left, right, li, ri, N, D, device); right = li = ri = None for a row table"""
    if isinstance(rows, (tuple, list)):
        if len(rows) != 4:
            raise ValueError("rows: an (N, D) tensor or a tuple (left, right, li, ri)")
        left = _f32_matrix("rows[0] (left)", rows[0], torch)
        dev, D = left.device, left.shape[1]
        right = _f32_matrix("rows[1] (right)", rows[1], torch, dev, D)
        index = []
        for name, v, table in (("li", rows[2], left), ("ri", rows[3], right)):
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.device != dev:
                raise ValueError("rows: %s must be a CUDA tensor on the pool's device" % name)
            if v.dtype is not torch.int32 or v.dim() != 1:
                raise ValueError("rows: %s must be a 1-D int32 tensor (got %s, shape %s)" % (name, v.dtype, tuple(v.shape)))
            if v.numel() and (int(v.min()) < 0 or int(v.max()) >= table.shape[0]):
                raise ValueError("rows: %s points outside its table of %d rows" % (name, table.shape[0]))
            index.append(v.contiguous())
        li, ri = index
        if li.numel() != ri.numel():
            raise ValueError("rows: li and ri differ in length (%d, %d)" % (li.numel(), ri.numel()))
        N = li.numel()
    else:
        left = _f32_matrix("rows", rows, torch)
        dev, D = left.device, left.shape[1]
        right = li = ri = None
        N = left.shape[0]
    return left, right, li, ri, N, D, dev


def _utility_vector(utility, N, dev, torch):
    if not isinstance(utility, torch.Tensor) or not utility.is_cuda or utility.device != dev:
        raise ValueError("utility: a CUDA tensor on the pool's device is needed")
    if utility.dtype is not torch.float32 or utility.dim() != 1 or utility.numel() != N:
        raise ValueError("utility: float32 of shape (%d,) is needed (got %s, shape %s)" % (N, utility.dtype, tuple(utility.shape)))
    return utility.contiguous()


def ranked_batch_device(rows, utility, labeled, n_instances, alpha=None):
    """Ranked batch selection of a pool on the GPU (alink_ranked_batch), Euclidean metric.

    rows         the pool: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri) — feature tables (., D) and int32
                 index vectors (N,): row n is |left[li[n]] - right[ri[n]]|, formed on the fly, never materialised
    utility      CUDA float32 (N,), larger = more informative (uncertainty.score_device, disagreement.score_members_device)
    labeled      CUDA float32 (M, D), M >= 1: the labelled rows, materialised (pairs as |l - r|)
    n_instances  batch size, clipped to N
    alpha        None: modAL's schedule (N - t) / (N + M); a number in [0, 1]: a fixed weight of the distance term
                 (0 = plain top-k order on the utility, 1 = farthest-point order)
    -> (idx int32 (k,), scores float32 (k,)) on the device: the picks in order and the score each had when picked; ties go
    to the lower index, a NaN utility never wins.  Nothing is synchronised or read back except, in the pair form, the
    range check of li / ri."""
    import torch
    from . import _abi, net_host
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    labeled = _f32_matrix("labeled", labeled, torch, dev, D)
    M = labeled.shape[0]
    if M == 0:
        raise ValueError("ranked_batch_device needs at least one labelled row: the cold start (the row nearest to all others) is "
                         "O(N^2 D) at pool scale and stays on the host (batch.ranked_batch)")
    utility = _utility_vector(utility, N, dev, torch)
    if alpha is not None and not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha = %r: None for the schedule, or a weight in [0, 1]" % (alpha,))
    if int(n_instances) < 1:
        raise ValueError("n_instances = %r must be at least 1" % (n_instances,))
    lib = _abi.init(dev.index or 0)
    k = min(int(n_instances), N)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_ranked_batch_scratch_bytes(N, int(n_instances)), dev)
    idx = torch.empty(max(k, 0), dtype=torch.int32, device=dev)
    scores = torch.empty(max(k, 0), dtype=torch.float32, device=dev)
    _abi.check(lib.alink_ranked_batch(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(labeled), M,
                                      _abi.ptr(utility), int(n_instances), -1.0 if alpha is None else float(alpha), _abi.ptr(idx),
                                      _abi.ptr(scores), sp, _abi.current_stream(dev)),
               "alink_ranked_batch")
    return idx, scores


def ranked_batch_cold_device(rows, utility, n_instances, alpha=None):
    """Ranked batch selection on the GPU WITHOUT labelled rows: modAL's cold start, then ranked_batch_device.

    Pick 0 is the pool's central row c, the row with the least mean Euclidean distance to all rows
    (density.information_density_device, want=("central",)); row c, materialised as (1, D), is the labelled set, and the pool
    without it goes to ranked_batch_device for the other n_instances - 1 picks, whose indices are mapped back
    (idx + (idx >= c)).  With a pool of N - 1 and one labelled row the schedule is alpha_t = (N - 1 - t) / N: the host
    ranked_batch's after its cold start.  The pair form drops position c from li / ri; the row form gathers the other
    N - 1 rows, which COPIES the table.  One scalar is read back (c: it decides what the second call is given), besides the
    pair form's range check of li / ri.

    rows, utility, n_instances, alpha as in ranked_batch_device.
    -> (idx int32 (k,), scores float32 (k,)) on the device, k = min(n_instances, N); scores[0] is NaN: the cold pick has no
    score."""
    import torch
    from . import density
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    utility = _utility_vector(utility, N, dev, torch)
    if alpha is not None and not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha = %r: None for the schedule, or a weight in [0, 1]" % (alpha,))
    if int(n_instances) < 1:
        raise ValueError("n_instances = %r must be at least 1" % (n_instances,))
    if N < 1:
        raise ValueError("ranked_batch_cold_device: the pool is empty")
    pool = left if li is None else (left, right, li, ri)
    central = density.information_density_device(pool, want=("central",))["central"]
    c = int(central)
    if c < 0:
        raise ValueError("ranked_batch_cold_device: no pool row has a mean distance that is a number")
    idx, scores = central, torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    if int(n_instances) > 1 and N > 1:
        keep = torch.cat((torch.arange(0, c, device=dev), torch.arange(c + 1, N, device=dev)))
        if li is None:
            labeled, rest = left[c:c + 1], left[keep]
        else:
            labeled = (left[li[c].long()] - right[ri[c].long()]).abs().unsqueeze(0)
            rest = (left, right, li[keep], ri[keep])
        more, more_scores = ranked_batch_device(rest, utility[keep], labeled, int(n_instances) - 1, alpha=alpha)
        more = more + (more >= c).to(torch.int32)                                # (a -1, nothing but NaN scores left, stays -1)
        idx, scores = torch.cat((idx, more)), torch.cat((scores, more_scores))
    return idx, scores
