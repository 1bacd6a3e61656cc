"""alfamix — ALFA-Mix queries (Parvaneh et al. 2022, "Active learning by feature mixing") through the pair scorer.  EXTENSION
(DESIGN.md §0, X15): the reference imports its strategies from modAL, which has no such sampler; no reference driver names this
one.

Every other strategy of this package scores a pair where it stands in feature space.  ALFA-Mix asks whether the scorer's
decision for the pair flips when its feature d = |l - r| is pulled a short way towards an anchor, the mean labelled row of a
class: such rows lie next to the decision surface in a direction that labelled data actually occupies.  The rule
(include/alink_hip.h, alink_head_feature_mix, states it in full), with z1, z2, z3 the head's pre-activations and yhat its
argmax (ties to class 0; one output: p > 0.5):

    u = (W3[:,0] - W3[:,1]) . [z2 > 0]    (one output: W3[:,0] . [z2 > 0])        v = (u W2^T) . [z1 > 0]        q = v W1^T
    g = q if yhat = 1 else -q             (one output: -q if yhat = 1 else q)     the direction that lowers yhat's margin
    per anchor a:   z = anchor_a - d,  s = eps |z| / |g|,  t = s g,  delta_e = min(max(t_e, min(z_e, 0)), max(z_e, 0))
                    mixed_a = d + delta       (delta = 0 when |g| == 0, or |g| or |z| is not finite)
    bit a of flip:  the argmax of the head on mixed_a differs from yhat

The step has length eps |z| along g and is kept, per element, between the row and the anchor: the paper's closed-form
alpha = eps |z| g / |g| (/) z clamped to [0, 1] and applied as d + alpha (.) z, without the division.  The batch rule: the
candidates are the rows with a flip under some anchor; with at least n of them, k-means over the candidates' rows from
k-means++ seeds, K = n, one query per cluster (cluster.py); picks still missing — fewer candidates than n, or an empty cluster —
are filled from the rows not yet picked by smallest |p0 - p1| (one output: |2p - 1|), ties to the lower index.  The paper fills
at random; here the fill is pinned.

`class_anchors`, `feature_mix`, `select`, `alfamix` are host float64 NumPy; `feature_mix_device` is alink_head_feature_mix
(alfamix.hip: the forward, the back-projection to the input and one more forward per anchor in one launch, no mixed row
written out unless asked for); `select_device`, `alfamix_device` keep the pool on the GPU; `alfamix_sampling` is modAL-shaped.
Not built: D > 512, a bf16-mode head, several ranks' pools in one call, learned alpha (the paper's optimised interpolation).
"""
import numpy as np

from . import cluster as _cluster
from . import egl as _egl
from .batch import _f32_matrix, _rows

DEVICE_OUTPUTS = ("probs", "flip", "mixed_probs", "mixed")
MAX_ANCHORS = 8                                            # one bit of the flip mask each
MAX_D = 512                                                # the mix holds a whole row in LDS


def class_anchors(rows, y, n_classes=2):
    """The anchors of a labelled set: the mean row of every class, in float64, rounded once to float32.  EXTENSION.
    rows: an (M, D) array or pair input [left, right] (rows |left - right|); y: M class indices, or an (M, C) one-hot / (M, 1)
    0-1 array.  An empty class gets no anchor.  -> float32 (A, D), A <= n_classes, in class order."""
    X = _rows(rows)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("rows: a non-empty (M, D) array of labelled rows is needed (got shape %s)" % (X.shape,))
    y = np.asarray(y)
    if y.ndim == 2:
        y = y.argmax(axis=1) if y.shape[1] > 1 else (y[:, 0] > 0.5)
    y = y.astype(np.int64).reshape(-1)
    if y.shape[0] != X.shape[0]:
        raise ValueError("y: %d labels for %d rows" % (y.shape[0], X.shape[0]))
    out = [X[y == c].mean(axis=0) for c in range(int(n_classes)) if (y == c).any()]
    if not out:
        raise ValueError("y: no label in 0 .. %d" % (int(n_classes) - 1))
    return np.stack(out).astype(np.float32)


def _check_anchors(anchors, D):
    A = np.asarray(anchors, np.float32)
    if A.ndim != 2 or not 1 <= A.shape[0] <= MAX_ANCHORS or A.shape[1] != D:
        raise ValueError("anchors: an (A, %d) array with A = 1 .. %d is needed (got shape %s)" % (D, MAX_ANCHORS, A.shape))
    return A


def _check_eps(eps):
    eps = float(eps)
    if not np.isfinite(eps) or eps < 0:
        raise ValueError("eps = %r must be finite and >= 0" % (eps,))
    return eps


def _logits(W, d):
    W1, b1, W2, b2, W3, b3 = W
    return np.maximum(np.maximum(d @ W1 + b1, 0) @ W2 + b2, 0) @ W3 + b3


def _softmax(z3):
    if z3.shape[1] > 1:
        e = np.exp(z3 - z3.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-z3))


def _argmax(p):
    return (p[:, 1] > p[:, 0]).astype(np.int64) if p.shape[1] == 2 else (p[:, 0] > 0.5).astype(np.int64)


def feature_mix(weights, X, anchors, eps=0.2):
    """The feature mix of every pair of X = [left, right] under the head `weights` = [W1, b1, W2, b2, W3, b3] (Keras order)
    towards every row of `anchors` (A, D), A <= 8, in host float64 NumPy: the rule of the module docstring.  EXTENSION.
    -> dict: probs (N, od), yhat int64 (N,), g (N, D), mixed (N, A, D), mixed_probs (N, A, od), margin (N, A) — the mixed row's
    logit margin of yhat (z3[yhat] - z3[1 - yhat]; one output: z3 if yhat = 1 else -z3) — and flip uint8 (N,), bit a set when
    the argmax on mixed[:, a] differs from yhat."""
    p, d, _, z1, _, z2, W2, W3 = _egl._host_pass(weights, X)
    W = [np.asarray(w, np.float64) for w in weights]
    eps = _check_eps(eps)
    An = _check_anchors(anchors, d.shape[1]).astype(np.float64)
    od = p.shape[1]
    yhat = _argmax(p)
    wd = W3[:, 0] - W3[:, 1] if od == 2 else W3[:, 0]
    u = wd[None, :] * (z2 > 0)
    v = (u @ W2.T) * (z1 > 0)
    q = v @ W[0].T
    sign = np.where(yhat == 1, 1.0, -1.0) if od == 2 else np.where(yhat == 1, -1.0, 1.0)
    g = sign[:, None] * q
    G = np.sqrt((g * g).sum(axis=1))
    N, A = len(d), len(An)
    mixed = np.empty((N, A, d.shape[1]))
    mixed_probs = np.empty((N, A, od))
    margin = np.empty((N, A))
    flip = np.zeros(N, np.uint8)
    for a in range(A):
        z = An[a][None, :] - d
        Z = np.sqrt((z * z).sum(axis=1))
        ok = (G != 0) & np.isfinite(G) & np.isfinite(Z)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = (eps * Z / G)[:, None] * g
            delta = np.minimum(np.maximum(t, np.minimum(z, 0)), np.maximum(z, 0))
        delta = np.where(ok[:, None], delta, 0.0)
        mixed[:, a] = d + delta
        z3 = _logits(W, mixed[:, a])
        pm = _softmax(z3)
        mixed_probs[:, a] = pm
        if od == 2:
            margin[:, a] = np.where(yhat == 1, z3[:, 1] - z3[:, 0], z3[:, 0] - z3[:, 1])
        else:
            margin[:, a] = np.where(yhat == 1, z3[:, 0], -z3[:, 0])
        flip |= ((_argmax(pm) != yhat).astype(np.uint8) << a).astype(np.uint8)
    return {"probs": p, "yhat": yhat, "g": g, "mixed": mixed, "mixed_probs": mixed_probs, "margin": margin, "flip": flip}


def _fill_value(probs):
    """|p0 - p1| (one column: |2p - 1|) in the probabilities' own precision: the smaller, the nearer the decision"""
    p = np.asarray(probs)
    if p.ndim != 2 or p.shape[1] not in (1, 2):
        raise ValueError("probs: an (N, 2) or (N, 1) array of the scorer's probabilities is needed (got shape %s)" % (p.shape,))
    return np.abs(p[:, 0] - p[:, 1]) if p.shape[1] == 2 else np.abs(p[:, 0] * p.dtype.type(2) - p.dtype.type(1))


def select(rows, flip, probs, n_instances, iters=10, random_state=None, exclude=None):
    """The batch rule on the host.  EXTENSION.

    rows          the (N, D) array of pool rows (pairs as |l - r|)
    flip          N flip masks (feature_mix's): a row with flip != 0 is a candidate
    probs         (N, 2) or (N, 1): the scorer's probabilities, for the fill
    n_instances   batch size, clipped to the rows that may be picked
    iters         Lloyd iterations of the k-means over the candidates (cluster.kmeans from badge.kmeans_pp seeds)
    random_state  the seed of np.random.RandomState for the seeding's uniforms
    exclude       None, or row indices that are never picked, as in cal.cal
    -> int64 (n,) picks: with at least n candidates the candidate nearest each final centre, in cluster order, else every
    candidate in index order; then the fill, by smallest |p0 - p1| (one column: |2p - 1|) among the rows not yet picked, ties
    to the lower index."""
    from .cal import _plan
    X = np.asarray(rows, np.float64)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    N = X.shape[0]
    flip = np.asarray(flip).reshape(-1)
    if flip.shape[0] != N:
        raise ValueError("flip: %d masks for %d rows" % (flip.shape[0], N))
    value = _fill_value(probs)
    if value.shape[0] != N:
        raise ValueError("probs: %d rows for a pool of %d" % (value.shape[0], N))
    n, ex = _plan(N, n_instances, exclude)
    free = np.ones(N, bool)
    free[ex] = False
    cand = np.flatnonzero((flip != 0) & free)
    if len(cand) >= n:
        near = _cluster._host_pick(X[cand], n, iters, random_state)
        picks = cand[near[near >= 0]]
    else:
        picks = cand
    free[picks] = False
    if len(picks) < n:
        v = np.where(free, value.astype(np.float64), np.inf)
        picks = np.concatenate([picks, np.argsort(v, kind="stable")[:n - len(picks)]])
    return picks.astype(np.int64)


def alfamix(weights, X, anchors, n_instances, eps=0.2, iters=10, random_state=None, exclude=None):
    """ALFA-Mix on the host: feature_mix, then select on the rows |left - right| of X = [left, right].  EXTENSION.
    -> (picks int64 (n,), info): info is feature_mix's dict."""
    info = feature_mix(weights, X, anchors, eps=eps)
    return select(_rows(X), info["flip"], info["probs"], n_instances, iters=iters, random_state=random_state, exclude=exclude), info


# ---- device forms ----------------------------------------------------------------------------------------------------------------
def feature_mix_device(head, L, R, anchors, li=None, ri=None, eps=0.2, want=("probs", "flip")):
    """The feature mix of a pool on the GPU (alink_head_feature_mix): one launch.  EXTENSION.

    head     a DenseHead in the float32 compute mode, D a multiple of 8 up to 512
    L, R     CUDA float32 (., D) feature tables on the head's device; without li / ri pair n is (L[n], R[n]), with them
             (L[li[n]], R[ri[n]]) — int32 (P,) index vectors, range-checked here, the pairs never materialised
    anchors  (A, D) float32, A = 1 .. 8: a CUDA tensor on the head's device, or an array (copied there)
    want     names among probs (P, od): DenseHead.predict_device's bits; flip uint8 (P,): bit a set when anchor a flips the
             decision; mixed_probs (P, A, od); mixed (P, A, D): the mixed rows themselves, for tests and diagnostics
    -> {name: CUDA tensor}.  Nothing is synchronised or read back except the range check of li / ri."""
    from . import _abi
    torch = head.torch
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in DEVICE_OUTPUTS]
    if unknown or not want:
        raise ValueError("unknown feature-mix output(s) %s: choose among %s" % (unknown, list(DEVICE_OUTPUTS)))
    dev = head._tdev
    L = _f32_matrix("L", L, torch, dev)
    if L.shape[1] != head.d_in:
        raise ValueError("L has D = %d, the head D = %d" % (L.shape[1], head.d_in))
    R = _f32_matrix("R", R, torch, dev, head.d_in)
    if (li is None) != (ri is None):
        raise ValueError("li and ri come together: both index vectors, or neither")
    if li is not None:
        li, ri = _egl._index_vector("li", li, L, torch, dev), _egl._index_vector("ri", ri, R, torch, dev)
        if li.numel() != ri.numel():
            raise ValueError("li and ri differ in length (%d, %d)" % (li.numel(), ri.numel()))
        P = li.numel()
    else:
        if L.shape[0] != R.shape[0]:
            raise ValueError("L and R differ in rows (%d, %d): without li / ri pair n is (L[n], R[n])" % (L.shape[0], R.shape[0]))
        P = L.shape[0]
    if head.compute_dtype != "f32":
        raise ValueError("feature_mix_device is the exact float32 form: the head is in the %s compute mode" % head.compute_dtype)
    if head.d_in % 8 or head.d_in > MAX_D:
        raise ValueError("the head has D = %d: the mix holds a whole row on chip, D a multiple of 8 up to %d" % (head.d_in, MAX_D))
    eps = _check_eps(eps)
    if isinstance(anchors, torch.Tensor):
        An = _f32_matrix("anchors", anchors, torch, dev, head.d_in)
        if not 1 <= An.shape[0] <= MAX_ANCHORS:
            raise ValueError("anchors: an (A, %d) tensor with A = 1 .. %d is needed (got shape %s)" % (head.d_in, MAX_ANCHORS, tuple(An.shape)))
    else:
        An = torch.from_numpy(np.array(_check_anchors(anchors, head.d_in), order="C")).to(dev)      # (a copy: the input may be read-only)
    A, od = An.shape[0], head.out_dim
    shapes = {"probs": (P, od), "flip": (P,), "mixed_probs": (P, A, od), "mixed": (P, A, head.d_in)}
    out = {w: torch.empty(shapes[w], dtype=torch.uint8 if w == "flip" else torch.float32, device=dev) for w in want}
    if P:
        _abi.check(head.lib.alink_head_feature_mix(head.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(li), _abi.ptr(ri), P, _abi.ptr(An), A, eps,
                                                   *[_abi.ptr(out.get(w)) for w in DEVICE_OUTPUTS], _abi.current_stream(head.device)),
                   "alink_head_feature_mix")
    return out


def select_device(rows, flip, probs, n_instances, iters=10, seed=None, exclude=None):
    """The batch rule on the GPU.  EXTENSION.

    rows         the pool as in cluster.kmeans_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri)
    flip         CUDA uint8 (N,), probs CUDA float32 (N, 2) or (N, 1): feature_mix_device's
    n_instances, iters, exclude  as in select; exclude: host integers; seed: the seed of the k-means++ uniforms (select's
                 random_state)
    The candidates' k-means is cluster.kmeans_sampling_device on (left, right, li[cand], ri[cand]) — no features copied — and the
    fill uncertainty.topk_device.  -> int32 (n,) picks on the device, in select's order.  The candidates' indices are read off
    the mask (torch.nonzero): the one synchronisation, which gives the candidate count that chooses the route."""
    import torch
    from . import uncertainty as _unc
    from .batch import _pool_rows
    from .cal import _plan
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if N < 1:
        raise ValueError("select_device: the pool is empty")
    if not isinstance(flip, torch.Tensor) or flip.device != dev or flip.dtype is not torch.uint8 or flip.shape != (N,):
        raise ValueError("flip: a uint8 (%d,) tensor on the pool's device is needed" % N)
    if not isinstance(probs, torch.Tensor) or probs.device != dev or probs.dtype is not torch.float32 or probs.dim() != 2 \
            or probs.shape[0] != N or probs.shape[1] not in (1, 2):
        raise ValueError("probs: a float32 (%d, 2) or (%d, 1) tensor on the pool's device is needed" % (N, N))
    n, ex = _plan(N, n_instances, exclude)
    free = torch.ones(N, dtype=torch.bool, device=dev)
    if len(ex):
        free[torch.from_numpy(ex).to(dev)] = False
    cand = torch.nonzero((flip != 0) & free).reshape(-1)                       # int64, ascending; synchronises
    c = int(cand.numel())
    value = (probs[:, 0] - probs[:, 1]).abs() if probs.shape[1] == 2 else (probs[:, 0] * 2 - 1).abs()
    if c >= n:
        sub = left.index_select(0, cand) if li is None else (left, right, li.index_select(0, cand), ri.index_select(0, cand))
        near, _ = _cluster.kmeans_sampling_device(sub, n, iters=iters, seed=seed)
        valid = near >= 0
        picked = cand.index_select(0, near.clamp(min=0).long())
        order = torch.sort((~valid).to(torch.int32), stable=True)[1]           # the clusters with a pick first, in cluster order
        picks = picked.index_select(0, order)
        m = valid.sum()
        taken = torch.zeros(N + 1, dtype=torch.bool, device=dev)               # slot N takes the empty clusters' writes
        taken[torch.where(valid, picked, torch.full_like(picked, N))] = True
        free = free & ~taken[:N]
    else:
        picks, m = cand, c
        free[cand] = False
        if c == n:
            return picks.to(torch.int32)
    fill, _ = _unc.topk_device(torch.where(free, value, torch.full_like(value, float("inf"))).contiguous(), n, largest=False)
    slot = torch.arange(n, device=dev)
    if picks.numel() < n:                                                       # fewer candidates than picks: pad to n slots
        picks = torch.cat([picks, picks.new_zeros(n - picks.numel())])
    return torch.where(slot < m, picks, fill.long().index_select(0, (slot - m).clamp(min=0))).to(torch.int32)


def alfamix_device(head, L, R, li, ri, anchors, n_instances, eps=0.2, iters=10, seed=None, exclude=None):
    """ALFA-Mix on the GPU: feature_mix_device, then select_device on the pairs' rows, formed on the fly.  EXTENSION.
    li = ri = None: pair n is (L[n], R[n]).  -> (picks int32 (n,) on the device, info): info holds "probs" and "flip" on the
    device.  The candidate count is read back to choose between the k-means route and the fill: the call's one synchronisation
    (beside the range check of li / ri)."""
    torch = head.torch
    info = feature_mix_device(head, L, R, anchors, li, ri, eps=eps, want=("probs", "flip"))
    if li is None:
        li = ri = torch.arange(L.shape[0], dtype=torch.int32, device=head._tdev)
    return select_device((L, R, li, ri), info["flip"], info["probs"], n_instances, iters=iters, seed=seed, exclude=exclude), info


def alfamix_sampling(classifier, X, n_instances=1, eps=0.2, random_state=None, iters=10):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=alfamix_sampling)): an ALFA-Mix batch of n_instances pairs of
    X = [left, right].  EXTENSION.  `classifier`: a learner whose estimator exposes siamese_net.get_weights() (egl.egl_sampling's
    rule) and which carries its labelled set as X_training / y_training: the anchors are class_anchors of it.  Nothing labelled
    yet: ValueError — there is nothing to mix towards.  CUDA tensors go through alfamix_device (the head must be a DenseHead:
    there is no fallback), anything else through alfamix.  -> (query_idx, instances): the instances as the other samplers of this
    package return them for pair input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    training, y = getattr(classifier, "X_training", None), getattr(classifier, "y_training", None)
    if training is None or y is None or len(y) == 0:
        raise ValueError("alfamix_sampling needs at least one labelled row: the anchors are the labelled classes' mean rows")
    net = _egl._head_of(classifier)
    if _cluster._is_cuda(training):
        training = [t.cpu().numpy() for t in training] if isinstance(training, (list, tuple)) else training.cpu().numpy()
    anchors = class_anchors(training, y.cpu().numpy() if hasattr(y, "cpu") else y)
    on_device = _cluster._is_cuda(X)
    if on_device:
        if not hasattr(net, "feature_mix_device"):
            raise TypeError("alfamix_sampling on CUDA tensors needs a DenseHead (got %s)" % type(net).__name__)
        picks, _ = alfamix_device(net, X[0], X[1], None, None, anchors, n_instances, eps=eps, iters=iters, seed=random_state)
        query_idx = picks.cpu().numpy().astype(np.int64)
    else:
        query_idx, _ = alfamix(net.get_weights(), X, anchors, n_instances, eps=eps, iters=iters, random_state=random_state)
    return query_idx, _cluster._instances(X, query_idx, on_device)
