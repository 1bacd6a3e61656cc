"""cal — Contrastive Active Learning (Margatina, Vernikos, Barrault & Aletras, EMNLP 2021, "Active Learning by Acquiring Contrastive
Examples") and the rectangular k-nearest-neighbour search it needs.  EXTENSION: the reference imports its
strategies from modAL, which has no such sampler; no reference driver names these.

The strategies before this one look at the pool alone (k-means, TypiClust, ProbCover) or at the scorer alone (the uncertainty
and committee measures, EGL, BADGE).  CAL asks which pool rows the scorer treats UNLIKE the labelled rows right next to them:
for every pool row take its k nearest labelled rows in feature space, score the row by the mean KL divergence between those
neighbours' predicted probabilities and its own, and query the largest scores.  A disguised or impostor pair sits among labelled
genuine pairs but is scored unlike them.

The neighbour rule (include/alink_hip.h, alink_knn_rect, states it in full) — typiclust.knn's with a second set:

    candidates  of query n: every reference row; no self-exclusion (the sets are different), no groups.  A reference whose squared
                norm is NaN or +inf in float32 is nobody's neighbour; a query whose own is has no neighbours
    score       score(n, j) = |c_j|^2 - 2 q_n . c_j  (= d2(n, j) - |q_n|^2); a score that is NaN or +inf never enters a list
    list        the k references of least (score, index), in that order: ties go to the lower index; `found` <= min(k, M) of
                them exist, unfilled slots hold index -1 and d2 NaN
    distance    d2 = |q_n - c_j|^2 by direct differences, for the winners only; a list is in the SCORE's order

The score rule (alink_cal_score), float64 throughout, every product and sum rounded once:

    p'_c   = p[n, c] if p[n, c] > 2^-126, else 2^-126
    kl(j)  = sum over c ascending of q[j, c] (log q[j, c] - log p'_c), over the classes with q[j, c] > 0 only
    score  = (sum over the slots ascending with idx >= 0 of kl(idx[n, slot])) / found, rounded to float32 once; 0 where found = 0

The direction is KL(neighbour || candidate), as in the authors' code.  Deliberate difference from that code: it works on
log-softmax outputs and so cannot meet a probability of zero; here probabilities come in as float32, where a softmax saturates
to exactly 0 and 1 — a neighbour's zero contributes nothing (the limit of q log q), and the candidate's is floored at 2^-126, the
least normal float32, which keeps the score finite (and large: such a row contradicts its neighbours as much as float32 can say).

`knn_rect`, `cal_scores` and `cal` are those rules in host float64 NumPy (an N x M matrix: small pools only); `knn_rect_device`,
`cal_scores_device` and `cal_device` are alink_knn_rect and alink_cal_score (knn_rect.hip: the N x M scores on the matrix cores,
never in memory, each lane's k best in registers) and uncertainty.topk_device.  Where nothing rounds, as on small-integer rows,
the lists agree bit for bit.

Not built: splitting the references over workgroups (a handful of queries against a huge gallery keeps few workgroups busy),
k > 32, groups, a cosine metric, several ranks' pools in one call.
"""
import numpy as np

from . import cluster as _cluster
from .batch import _rows
from .typiclust import MAX_K_NN, _check_k, _labelled_indices

MAX_CLASSES = 32                                           # classes of a device score (CAL_MAX_C, knn_rect.hip)
P_FLOOR = 2.0 ** -126                                      # the least normal float32


def _host_rows(name, rows):
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("%s: a non-empty (rows, D) array is needed (got shape %s)" % (name, X.shape))
    return X


def knn_rect(queries, references, k):
    """The k nearest rows of the (M, D) array `references` for every row of the (N, D) array `queries`, on the host: the
    neighbour rule of the module docstring in float64.  EXTENSION.
    -> (idx int32 (N, k) indices into `references`, d2 float64 (N, k), found int32 (N,))."""
    Q, Cm = _host_rows("queries", queries), _host_rows("references", references)
    if Q.shape[1] != Cm.shape[1]:
        raise ValueError("queries have D = %d, references D = %d" % (Q.shape[1], Cm.shape[1]))
    k = _check_k(k)
    N, M = len(Q), len(Cm)
    with np.errstate(invalid="ignore", over="ignore"):
        qn, cn = (Q * Q).sum(axis=1), (Cm * Cm).sum(axis=1)
        q_alive, c_alive = np.isfinite(qn.astype(np.float32)), np.isfinite(cn.astype(np.float32))
        score = cn[None, :] - 2.0 * (np.where(q_alive[:, None], Q, 0.0) @ np.where(c_alive[:, None], Cm, 0.0).T)
        score = np.where(q_alive[:, None] & c_alive[None, :] & (score < np.inf), score, np.inf)
    w = min(k, M)
    order = np.argsort(score, axis=1, kind="stable")[:, :w]                 # ties to the lower index
    real = np.take_along_axis(score, order, axis=1) < np.inf
    idx = np.full((N, k), -1, np.int32)
    idx[:, :w] = np.where(real, order, -1)
    d2 = np.full((N, k), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        d2[:, :w] = np.where(real, ((Q[:, None, :] - Cm[order]) ** 2).sum(axis=2), np.nan)
    return idx, d2, real.sum(axis=1).astype(np.int32)


def _host_probs(name, p, C=None):
    P = np.asarray(p, np.float64)
    if P.ndim != 2 or P.shape[0] < 1 or P.shape[1] < 1:
        raise ValueError("%s: a non-empty (rows, C) array of probabilities is needed (got shape %s)" % (name, P.shape))
    if C is not None and P.shape[1] != C:
        raise ValueError("%s has C = %d classes, the pool's probabilities C = %d" % (name, P.shape[1], C))
    return P


def cal_scores(p_pool, p_labelled, idx):
    """The CAL score of every pool row on the host, the score rule of the module docstring.  EXTENSION.
    p_pool (N, C) and p_labelled (M, C): predicted probabilities; idx (N, k): knn_rect's lists (-1: an unfilled slot).
    -> float32 (N,).  ValueError for an index >= M."""
    P = _host_probs("p_pool", p_pool)
    Qm = _host_probs("p_labelled", p_labelled, P.shape[1])
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape[0] != len(P) or idx.shape[1] < 1 or idx.dtype.kind not in "iu":
        raise ValueError("idx: an integer (%d, k) array is needed (got shape %s, %s)" % (len(P), idx.shape, idx.dtype))
    if idx.max() >= len(Qm):
        raise ValueError("idx: a neighbour index outside the %d labelled rows" % len(Qm))
    N, C = P.shape
    log_p = np.log(np.where(P > P_FLOOR, P, P_FLOOR))
    with np.errstate(divide="ignore", invalid="ignore"):
        log_q = np.log(Qm)
    total, found = np.zeros(N), np.zeros(N, np.int64)
    for s in range(idx.shape[1]):                                          # ascending slot order
        valid = idx[:, s] >= 0
        j = np.where(valid, idx[:, s], 0)
        kl = np.zeros(N)
        for c in range(C):                                                 # ascending class order
            q = Qm[j, c]
            with np.errstate(invalid="ignore"):
                kl = kl + np.where(q > 0, q * (log_q[j, c] - log_p[:, c]), 0.0)
        total = total + np.where(valid, kl, 0.0)
        found += valid
    return np.where(found > 0, total / np.maximum(found, 1), 0.0).astype(np.float32)


def _plan(N, n_instances, exclude):
    """-> (the batch size, clipped to the rows that may be picked; the excluded rows int64)"""
    n = _cluster._check_instances(n_instances)
    ex = _labelled_indices(exclude, N)
    if N - len(ex) < 1:
        raise ValueError("every one of the %d rows is excluded" % N)
    return min(n, N - len(ex)), ex


def cal(rows, labelled_rows, p_pool, p_labelled, n_instances, k_nn=10, exclude=None):
    """Contrastive Active Learning on the host: the n_instances rows of the (N, D) array `rows` with the largest CAL score
    against the (M, D) array `labelled_rows`, everything in float64 NumPy.  EXTENSION.

    p_pool, p_labelled  the scorer's probabilities for both sets, (N, C) and (M, C)
    n_instances         batch size, clipped to the rows that may be picked
    exclude             None, or row indices into `rows` that are never picked (their scores count as -inf)
    -> (picks int64, scores float32 (N,)): the picks by score descending, ties to the lower index — the order
    uncertainty.topk_device gives; `scores` are cal_scores', unmasked."""
    Q = _host_rows("rows", rows)
    n, ex = _plan(len(Q), n_instances, exclude)
    idx, _, _ = knn_rect(Q, labelled_rows, k_nn)
    scores = cal_scores(p_pool, p_labelled, idx)
    value = scores.astype(np.float64)
    value[ex] = -np.inf
    return np.argsort(-value, kind="stable")[:n].astype(np.int64), scores


# ---- device forms -------------------------------------------------------------------------------------------------------------
def _two_sets(queries, references, what):
    import torch
    from .batch import _pool_rows
    ql, qr, qli, qri, N, D, dev = _pool_rows(queries, torch)
    cl, cr, cli, cri, M, Dc, cdev = _pool_rows(references, torch)
    if (qli is None) != (cli is None):
        raise ValueError("%s: queries and references are both (rows, D) tensors or both (left, right, li, ri) tuples — materialise "
                         "the smaller side" % what)
    if cdev != dev:
        raise ValueError("%s: the references are on %s, the queries on %s" % (what, cdev, dev))
    if Dc != D:
        raise ValueError("%s: the references have D = %d, the queries D = %d" % (what, Dc, D))
    if N < 1 or M < 1:
        raise ValueError("%s: %s empty" % (what, "the queries are" if N < 1 else "the references are"))
    if D > _cluster.MAX_D:
        raise ValueError("rows have D = %d columns, beyond the %d a device row may have" % (D, _cluster.MAX_D))
    return (ql, qr, qli, qri), (cl, cr, cli, cri), N, M, D, dev


def knn_rect_device(queries, references, k):
    """The k nearest reference rows of every query row on the GPU (alink_knn_rect).  EXTENSION.

    queries, references  each as typiclust.knn_device takes a pool: a CUDA float32 (., D) tensor, or a tuple (left, right, li, ri);
                         BOTH tensors or BOTH tuples (which may share their tables)
    k                    1 .. 32
    -> (idx int32 (N, k) indices into the references, d2 float32 (N, k), found int32 (N,)) on the device.  Nothing is synchronised
    or read back except, in the pair form, the range check of li / ri."""
    import torch
    from . import _abi, net_host
    q, c, N, M, D, dev = _two_sets(queries, references, "knn_rect_device")
    k = _check_k(k)
    if k > MAX_K_NN:
        raise ValueError("k = %d beyond the %d neighbours a device call keeps" % (k, MAX_K_NN))
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_knn_rect_scratch_bytes(N, M, D, k), dev)
    idx = torch.empty((N, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((N, k), dtype=torch.float32, device=dev)
    found = torch.empty(N, dtype=torch.int32, device=dev)
    _abi.check(lib.alink_knn_rect(*([_abi.ptr(t) for t in q] + [N] + [_abi.ptr(t) for t in c] + [M, D, k, _abi.ptr(idx), _abi.ptr(d2),
                                                                                               _abi.ptr(found), sp, _abi.current_stream(dev)])),
               "alink_knn_rect")
    return idx, d2, found


def _probs(name, p, torch, dev=None, C=None):
    if not isinstance(p, torch.Tensor) or not p.is_cuda or p.dtype is not torch.float32 or p.dim() != 2 or p.shape[0] < 1:
        raise ValueError("%s: a non-empty CUDA float32 (rows, C) tensor of probabilities is needed" % name)
    if dev is not None and p.device != dev:
        raise ValueError("%s is on %s, the pool's probabilities on %s" % (name, p.device, dev))
    if C is not None and p.shape[1] != C:
        raise ValueError("%s has C = %d classes, the pool's probabilities C = %d" % (name, p.shape[1], C))
    if not 1 <= p.shape[1] <= MAX_CLASSES:
        raise ValueError("%s has C = %d classes, outside the 1 .. %d a device score takes" % (name, p.shape[1], MAX_CLASSES))
    return p.contiguous()


def cal_scores_device(p_pool, p_labelled, idx):
    """The CAL score of every pool row on the GPU (alink_cal_score): float64 arithmetic on the device.  EXTENSION.
    p_pool CUDA float32 (N, C), p_labelled CUDA float32 (M, C), C <= 32; idx CUDA int32 (N, k), k <= 32: knn_rect_device's lists.
    An index >= M is the caller's error: such a slot is skipped like an unfilled one (the host form raises).
    -> float32 (N,) on the device.  Nothing is synchronised or read back."""
    import torch
    from . import _abi
    P = _probs("p_pool", p_pool, torch)
    Qm = _probs("p_labelled", p_labelled, torch, P.device, P.shape[1])
    N, C = P.shape
    if not isinstance(idx, torch.Tensor) or idx.device != P.device or idx.dtype is not torch.int32 or idx.dim() != 2 or idx.shape[0] != N \
            or not 1 <= idx.shape[1] <= MAX_K_NN:
        raise ValueError("idx: an int32 (%d, k) tensor, k = 1 .. %d, on the probabilities' device is needed" % (N, MAX_K_NN))
    idx = idx.contiguous()
    lib = _abi.init(P.device.index or 0)
    score = torch.empty(N, dtype=torch.float32, device=P.device)
    _abi.check(lib.alink_cal_score(_abi.ptr(P), _abi.ptr(Qm), C, _abi.ptr(idx), N, Qm.shape[0], idx.shape[1], _abi.ptr(score),
                                   _abi.current_stream(P.device)), "alink_cal_score")
    return score


def cal_device(rows, labelled_rows, p_pool, p_labelled, n_instances, k_nn=10, exclude=None):
    """Contrastive Active Learning on the GPU: knn_rect_device, cal_scores_device, uncertainty.topk_device.  EXTENSION.

    rows, labelled_rows  the pool and the labelled set as knn_rect_device takes queries and references
    p_pool, p_labelled   CUDA float32 (N, C) and (M, C): the scorer's probabilities for both sets
    n_instances, exclude as in cal; exclude: host integers
    -> (picks int32 (n,) on the device, info): the picks by score descending, ties to the lower index; info holds "scores"
    (float32 (N,), unmasked), "idx" (int32 (N, k_nn)), "d2" and "found", all on the device.  Nothing is synchronised or read back
    except, in the pair form, the range check of li / ri."""
    import torch
    from . import uncertainty as _unc
    _cluster._check_instances(n_instances)
    idx, d2, found = knn_rect_device(rows, labelled_rows, k_nn)            # (checks both sets)
    N, dev = idx.shape[0], idx.device
    n, ex = _plan(N, n_instances, exclude)
    scores = cal_scores_device(p_pool, p_labelled, idx)
    value = scores
    if len(ex):
        value = scores.clone()
        value[torch.from_numpy(ex).to(dev)] = float("-inf")
    picks, _ = _unc.topk_device(value, n)
    return picks, {"scores": scores, "idx": idx, "d2": d2, "found": found}


def cal_sampling(classifier, X, n_instances=1, k_nn=10):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=cal_sampling)): the n_instances rows of X, an (N, D) array or pair
    input [left, right] (rows |left - right|), with the largest CAL score against the learner's labelled rows.  EXTENSION.
    The labelled rows are `classifier.X_training`, as batch.uncertainty_batch_sampling takes them (array or pair list); both
    probability sets come from `classifier.predict_proba`.  Nothing labelled yet: ValueError, as batch.ranked_batch_device raises
    without a labelled row — there is nothing to contrast with.  CUDA tensors go through cal_device, anything else through cal.
    -> (query_idx, instances): the instances as the other samplers of this package return them for pair input,
    `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    training = getattr(classifier, "X_training", None)
    if training is None:
        raise ValueError("cal_sampling needs at least one labelled row: the score contrasts a pool row with its labelled neighbours")
    p_pool, p_lab = classifier.predict_proba(X), classifier.predict_proba(training)
    on_device = _cluster._is_cuda(X)
    if on_device:
        import torch
        rows = (X[0] - X[1]).abs() if isinstance(X, (list, tuple)) else X
        if _cluster._is_cuda(training):
            labelled = (training[0] - training[1]).abs() if isinstance(training, (list, tuple)) else training
        else:
            labelled = torch.from_numpy(_rows(training).astype(np.float32)).to(rows.device)

        def dev_probs(p):
            p = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(p, np.float32)))
            return p.to(rows.device, torch.float32)
        picks, _ = cal_device(rows, labelled.to(torch.float32), dev_probs(p_pool), dev_probs(p_lab), n_instances, k_nn=k_nn)
        query_idx = picks.cpu().numpy().astype(np.int64)
    else:
        query_idx, _ = cal(_rows(X), _rows(training), np.asarray(p_pool), np.asarray(p_lab), n_instances, k_nn=k_nn)
    return query_idx, _cluster._instances(X, query_idx, on_device)
