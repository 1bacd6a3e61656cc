"""bait — BAIT batches (Ash, Goel, Krishnamurthy & Kakade 2021, "Gone Fishing: Neural Active Learning with Fisher Embeddings"):
a batch chosen by the Fisher information it adds.  EXTENSION: the reference imports its strategies from modAL,
which has no such sampler; no reference driver names this one.

BADGE (badge.py) spreads its picks over the gradient embeddings with a random draw.  BAIT picks, one row after another, the row
that most reduces tr(M^-1 Phi): Phi is the Fisher matrix of the whole pool, M the Fisher matrix of what is labelled plus what is
picked so far.  It over-samples `over` x k rows forward and prunes back to k.

For the pair head the rule collapses.  The last layer's per-label gradients of a pair are collinear — two outputs:
grad l(x, 0) = p1 s, grad l(x, 1) = -p0 s with s = [-a2 ; a2] — so the per-sample Fisher is the rank-one p0 p1 s s^T, everything
lives in the span of [-I ; I] / sqrt 2, and BAIT over the 2 h2-dimensional embedding with the paper's rank-two trace expression
equals BAIT over F = h2 dimensions with ONE factor row per pair and the same ridge (tests/test_bait_host.py checks the two
scores against each other; DESIGN.md §9 derives it).  The pinned rule (include/alink_hip.h states the device arithmetic in full):

    factor    f is (N, F = h2), from the head's probs and emb as alink_head_egl writes them; yhat is egl's, c* the other class.
              two outputs: f_nj = emb[n, c* h2 + j] * float32(sqrt(2 p_yhat / p_c*))            (= sqrt(2 p0 p1) a2)
              one output:  f_nj = |emb[n, j]| * float32(sqrt(p (1 - p)) / |p - [p > 0.5]|)      (= sqrt(p (1 - p)) a2)
              the scale in float64 from the float32 probabilities, rounded once; a saturated row (an output outside
              [1e-7, 1 - 1e-7]; its emb is zero already) has f = 0; the bias column is not part of the Fisher
    blocks    a row may carry m factors side by side, a table (N, m F): independent committee members give a block-diagonal
              Fisher and the score is the sum of the members' scores, each against its own A, B.  m = 1 is plain BAIT.
              F a multiple of 8, 8 <= F <= 128, 1 <= m <= 8, m F <= 512 (the device's limits)
    Gram      Phi_j = (1 / N_all) sum over pool + labelled of f_j f_j^T;  M0_j = lam I + sum over the labelled of f_j f_j^T,
              lam = 1;  B0 = M0^-1 by np.linalg.inv in float64 on the host (the device route reads the factor rows back once
              and forms the Gram matrices on the host too: a device Gram kernel is not built)
    forward   t = 0 .. min(over k, free rows) - 1:  score_n = sum over blocks of q_A / (1 + q_B), q_A = f^T A f, q_B = f^T B f,
              B = M^-1, A = B Phi B (recomputed from B and Phi at every step: a function of the state alone);  pick the free row
              of largest score, ties to the lower index, a NaN never wins, labelled rows are never free;  then per block
              w = B f, B <- B - w w^T / (1 + f^T w)
    backward  while more than k rows are kept: among them score = sum over blocks of q_A / (q_B - 1), a row with any q_B >= 1
              is skipped; remove the row of largest score, ties to the earlier pick; B <- B + w w^T / (1 - f^T w).  If every
              row is skipped nothing more is removed and the first k kept rows are the result.  The result is the kept rows in
              the order they were picked.
    Deliberately not the authors' code: no nLabeled / (nLabeled + K) rescaling of M0; deterministic ties.

`fisher_factor`, `fisher_matrix`, `bait_scores`, `bait_select`, `bait` are host float64 NumPy; `fisher_factor_device`,
`bait_scores_device`, `bait_select_device`, `bait_device` run on the GPU (bait.hip: the score pass is two
small-matrix MFMA products per block and pick, the update one one-workgroup launch in float64, the whole loop enqueued without a
host synchronisation); `bait_sampling` is modAL-shaped.  Not built: per-sample rank above one (another head, or more layers than
the last); an incrementally updated score (q' = q - (f . w)^2 / c ...), which does 8 x less work but makes a row's float32 score
depend on the pick history — here a row's score is a function of (A, B, f_n) alone, and the tests rest on that.
"""
import numpy as np

from . import egl as _egl

TILE = 128                                                 # ALINK_BAIT_TILE: rows per partial maximum of alink_bait_scores
MAX_F, MAX_BLOCKS, MAX_WIDTH = 128, 8, 512


def _check_shape(F, blocks):
    if F % 8 or not 8 <= F <= MAX_F or not 1 <= blocks <= MAX_BLOCKS or blocks * F > MAX_WIDTH:
        raise ValueError("F = %d, blocks = %d: F a multiple of 8 in 8 .. %d, 1 .. %d blocks, blocks x F <= %d"
                         % (F, blocks, MAX_F, MAX_BLOCKS, MAX_WIDTH))


def _blocks_of(f, blocks):
    """(N, m F) -> (m, N, F) views"""
    f = np.asarray(f)
    if f.ndim != 2 or int(blocks) < 1 or f.shape[1] % int(blocks):
        raise ValueError("f: an (N, blocks x F) table is needed (got shape %s, blocks = %r)" % (f.shape, blocks))
    return f.reshape(f.shape[0], int(blocks), -1).transpose(1, 0, 2)


# ---- host, float64 ---------------------------------------------------------------------------------------------------------
def fisher_factor(weights, X):
    """The ideal Fisher factor of every pair of X = [left, right] under the head `weights` (Keras order): sqrt(2 p0 p1) a2 for
    the two-output head, sqrt(p (1 - p)) a2 for the one-output head, 0 on a saturated row.  EXTENSION.  -> (N, h2) float64."""
    p, _, _, _, a2, _, _, _ = _egl._host_pass(weights, X)
    s = np.sqrt(2 * p[:, 0] * p[:, 1]) if p.shape[1] == 2 else np.sqrt(p[:, 0] * (1 - p[:, 0]))
    return np.where(_egl._inside(p), s, 0.0)[:, None] * a2


def factor_from_outputs(probs, emb, dtype=np.float64):
    """The factor rule of the module docstring applied to given head outputs (egl's probs (N, od) and emb (N, od h2)) with the
    row product in `dtype`: float64 is the reference of the device's rows, float32 a restatement of what the device computes.
    The scale is float64 from the probabilities as given, rounded once to float32, as on the device."""
    probs, emb = np.asarray(probs), np.asarray(emb)
    od = probs.shape[1]
    h2 = emb.shape[1] // od
    p = probs.astype(np.float64)
    lo, hi = np.float32(1e-7), np.float32(1) - np.float32(1e-7)
    inside = ((probs >= lo) & (probs <= hi)).all(axis=1)
    n = np.arange(len(p))
    with np.errstate(divide="ignore", invalid="ignore"):
        if od == 2:
            yhat = (probs[:, 1] > probs[:, 0]).astype(int)
            scale = np.sqrt(2.0 * p[n, yhat] / p[n, 1 - yhat])
            rows = emb.reshape(len(p), 2, h2)[n, 1 - yhat]
        else:
            scale = np.sqrt(p[:, 0] * (1.0 - p[:, 0])) / np.abs(p[:, 0] - (probs[:, 0] > 0.5))
            rows = np.abs(emb)
    scale = np.where(inside, scale, 0.0).astype(np.float32)
    return np.where(inside[:, None], rows.astype(dtype) * scale.astype(dtype)[:, None], 0).astype(dtype)


def fisher_matrix(f, rows=None, scale=1.0, blocks=1):
    """scale x the sum of f_j f_j^T over all rows (or over `rows`), per block.  EXTENSION.  -> (blocks, F, F) float64."""
    fb = _blocks_of(np.asarray(f, np.float64), blocks)
    if rows is not None:
        fb = fb[:, np.asarray(rows, np.int64)]
    return (fb.transpose(0, 2, 1) @ fb) * float(scale)


def bait_scores(f, A, B, sign=1, blocks=1, dtype=np.float64):
    """score of every row against A, B (blocks, F, F): the sum over blocks of q_A / (1 + q_B) (sign +1) or q_A / (q_B - 1)
    (sign -1; NaN for a row with any q_B >= 1), in `dtype`.  EXTENSION.  -> (N,)"""
    fb = _blocks_of(np.asarray(f, dtype), blocks)
    out, skip = None, np.zeros(fb.shape[1], bool)
    for j in range(fb.shape[0]):
        qa = ((fb[j] @ np.asarray(A[j], dtype)) * fb[j]).sum(axis=1, dtype=dtype)
        qb = ((fb[j] @ np.asarray(B[j], dtype)) * fb[j]).sum(axis=1, dtype=dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = qa / (dtype(1) + qb) if sign > 0 else qa / (qb - dtype(1))
        if sign < 0:
            skip |= qb >= 1
        out = term if out is None else out + term
    return np.where(skip, dtype(np.nan), out) if sign < 0 else out


def woodbury(B, f_row, sign=1, blocks=1):
    """B after adding (sign +1) or removing (sign -1) the row's rank-one terms: B - w w^T / (1 + f^T w), B + w w^T / (1 - f^T w)
    per block, float64.  -> a new (blocks, F, F) array"""
    B = np.array(B, np.float64)
    fr = np.asarray(f_row, np.float64).reshape(int(blocks), -1)
    for j in range(B.shape[0]):
        w = B[j] @ fr[j]
        fw = fr[j] @ w
        B[j] -= np.outer(w, w) / ((1.0 + fw) if sign > 0 else (fw - 1.0))
    return B


def first_argmax(scores, allowed):
    """the allowed row of largest score, ties to the lower index, a NaN never wins (-inf may); -1 when there is none"""
    scores = np.asarray(scores)
    cand = np.flatnonzero(np.asarray(allowed, bool) & ~np.isnan(scores))
    return int(cand[np.argmax(scores[cand])]) if len(cand) else -1


def bait_select(f, phi, M0, k, over=2, blocks=1, free=None):
    """BAIT's forward selection and backward prune over the factor rows f (N, blocks x F), the rule of the module docstring in
    float64.  EXTENSION.

    phi, M0   (blocks, F, F) (or (F, F) for one block): the pool's Fisher matrix and the ridge plus the labelled rows'
    k         rows to return, clipped to the free rows;  over: the forward phase picks over x k
    free      None: every row; else a boolean (N,) mask, False on the labelled rows
    -> (idx int64 (k,) in pick order, B (blocks, F, F): the running inverse after the prune)"""
    f = np.asarray(f, np.float64)
    m = int(blocks)
    fb = _blocks_of(f, m)
    F = fb.shape[2]
    phi, M0 = np.asarray(phi, np.float64).reshape(m, F, F), np.asarray(M0, np.float64).reshape(m, F, F)
    if int(k) < 1:
        raise ValueError("k = %r must be at least 1" % (k,))
    if int(over) < 1:
        raise ValueError("over = %r must be at least 1" % (over,))
    free = np.ones(len(f), bool) if free is None else np.array(free, bool)
    if free.shape != (len(f),):
        raise ValueError("free: a boolean mask of %d rows is needed (got shape %s)" % (len(f), free.shape))
    k = min(int(k), int(free.sum()))
    if k < 1:
        raise ValueError("bait_select: no free row")
    B = np.stack([np.linalg.inv(M0[j]) for j in range(m)])
    picked = []
    for _ in range(min(int(over) * k, int(free.sum()))):
        A = np.stack([B[j] @ phi[j] @ B[j] for j in range(m)])
        n = first_argmax(bait_scores(f, A, B, 1, m), free)
        if n < 0:
            break
        picked.append(n)
        free[n] = False
        B = woodbury(B, f[n], 1, m)
    kept = list(picked)
    while len(kept) > k:
        A = np.stack([B[j] @ phi[j] @ B[j] for j in range(m)])
        r = first_argmax(bait_scores(f[kept], A, B, -1, m), np.ones(len(kept), bool))
        if r < 0:
            break
        B = woodbury(B, f[kept[r]], -1, m)
        del kept[r]
    return np.asarray(kept[:k], np.int64), B


def _labelled(labelled, N):
    from .typiclust import _labelled_indices
    return _labelled_indices(labelled, N)


def bait(weights, X, labelled, n_instances, lam=1.0, over=2):
    """A BAIT batch of n_instances pairs of X = [left, right] on the host: fisher_factor, Phi over all rows, M0 = lam I + the
    labelled rows' sum, bait_select over the rows not in `labelled` (row indices, or None).  EXTENSION.  -> idx int64 (k,)"""
    f = fisher_factor(weights, X)
    lab = _labelled(labelled, len(f))
    free = np.ones(len(f), bool)
    free[lab] = False
    phi = fisher_matrix(f, scale=1.0 / len(f))
    M0 = float(lam) * np.eye(f.shape[1])[None] + fisher_matrix(f, rows=lab)
    return bait_select(f, phi, M0, n_instances, over=over, free=free)[0]


def pack_ab(A, B):
    """float32 images of A and B (blocks, F, F) as alink_bait_scores reads them: per block A's image, then B's, element (k, c)
    of a matrix at ((k // 8) F + c) 8 + (k % 2) 4 + (k % 8) // 2.  -> float32 (blocks, 2, F F)"""
    A, B = np.asarray(A), np.asarray(B)
    m, F = A.shape[0], A.shape[1]
    k, c = np.meshgrid(np.arange(F), np.arange(F), indexing="ij")
    at = (((k // 8) * F + c) * 8 + (k % 2) * 4 + (k % 8) // 2).reshape(-1)
    out = np.zeros((m, 2, F * F), np.float32)
    for j in range(m):
        out[j, 0, at] = np.asarray(A[j], np.float32).reshape(-1)
        out[j, 1, at] = np.asarray(B[j], np.float32).reshape(-1)
    return out


# ---- device ------------------------------------------------------------------------------------------------------------------
def _table(name, f, torch, blocks):
    if not isinstance(f, torch.Tensor) or not f.is_cuda or f.dtype is not torch.float32 or f.dim() != 2:
        raise ValueError("%s must be a CUDA float32 (N, blocks x F) tensor" % name)
    if f.shape[0] < 1 or int(blocks) < 1 or f.shape[1] % int(blocks):
        raise ValueError("%s: a non-empty (N, blocks x F) table is needed (got shape %s, blocks = %r)" % (name, tuple(f.shape), blocks))
    _check_shape(f.shape[1] // int(blocks), int(blocks))
    return f.contiguous(), f.shape[0], f.shape[1] // int(blocks)


def fisher_factor_device(probs, emb):
    """The factor rows of a pool on the GPU from alink_head_egl's outputs (alink_fisher_factor).  EXTENSION.
    probs (P, od), emb (P, od h2): CUDA float32, as egl.expected_gradient_length_device returns them -> (P, h2) float32."""
    import torch
    from . import _abi
    if not (isinstance(probs, torch.Tensor) and isinstance(emb, torch.Tensor) and probs.is_cuda and emb.device == probs.device
            and probs.dtype is torch.float32 and emb.dtype is torch.float32 and probs.dim() == 2 and emb.dim() == 2):
        raise ValueError("probs and emb must be CUDA float32 matrices on one device")
    P, od = probs.shape
    if od not in (1, 2) or emb.shape[0] != P or emb.shape[1] % od:
        raise ValueError("probs %s and emb %s do not belong together" % (tuple(probs.shape), tuple(emb.shape)))
    h2 = emb.shape[1] // od
    dev = probs.device
    lib = _abi.init(dev.index or 0)
    f = torch.empty((P, h2), dtype=torch.float32, device=dev)
    _abi.check(lib.alink_fisher_factor(_abi.ptr(probs.contiguous()), _abi.ptr(emb.contiguous()), P, od, h2, _abi.ptr(f),
                                       _abi.current_stream(dev)), "alink_fisher_factor")
    return f


def _free_mask(free, N, torch, dev):
    if not isinstance(free, torch.Tensor) or free.device != dev or free.dtype is not torch.uint8 or free.shape != (N,):
        raise ValueError("free must be a uint8 CUDA tensor of %d rows on f's device (1: the row may be picked)" % N)
    if not free.is_contiguous():
        raise ValueError("free must be contiguous: it is updated in place")
    return free


def bait_scores_device(f, AB, free, sign=1, blocks=1, want_scores=True):
    """One score pass on the GPU (alink_bait_scores).  EXTENSION.  f: CUDA float32 (N, blocks x F); AB: pack_ab's images as a CUDA
    float32 tensor; free: uint8 (N,) -> (scores float32 (N,) or None, partial int32 (ceil(N / TILE), 2): per tile the best free
    row's score (the float32's bits) and index, (-inf, 2^31 - 1) without one)."""
    import torch
    from . import _abi
    f, N, F = _table("f", f, torch, blocks)
    dev = f.device
    free = _free_mask(free, N, torch, dev)
    if not isinstance(AB, torch.Tensor) or AB.device != dev or AB.dtype is not torch.float32 or AB.numel() != int(blocks) * 2 * F * F:
        raise ValueError("AB: pack_ab's float32 images of %d blocks on f's device" % int(blocks))
    if sign not in (1, -1):
        raise ValueError("sign = %r: +1 forward, -1 backward" % (sign,))
    AB = AB.contiguous()
    lib = _abi.init(dev.index or 0)
    scores = torch.empty(N, dtype=torch.float32, device=dev) if want_scores else None
    partial = torch.empty(((N + TILE - 1) // TILE, 2), dtype=torch.int32, device=dev)
    _abi.check(lib.alink_bait_scores(_abi.ptr(f), N, F, int(blocks), _abi.ptr(AB), _abi.ptr(free), int(sign), _abi.ptr(scores),
                                     _abi.ptr(partial), _abi.current_stream(dev)), "alink_bait_scores")
    return scores, partial


def best_of_partials(partial):
    """(score, index) of bait_scores_device's partial maxima: the largest score, ties to the lower index; (-inf, -1) for none"""
    p = partial.cpu().numpy()
    v, i = p[:, 0].copy().view(np.float32), p[:, 1]
    t = int(np.argmax(v))                                  # tiles ascend in index: the first maximum is the lowest index
    return (float(v[t]), int(i[t])) if i[t] != 0x7fffffff else (float("-inf"), -1)


def bait_select_device(f, phi, B, free, k_forward, k_keep, blocks=1):
    """The forward picks and the backward prune on the GPU (alink_bait_select), enqueued without a host synchronisation.  EXTENSION.

    f        CUDA float32 (N, blocks x F)
    phi, B   CUDA float64 (blocks, F, F), symmetric; B = M0^-1 comes back as the running inverse (in place)
    free     uint8 (N,): 1 where a row may be picked; the rows returned are cleared in place
    k_forward, k_keep   forward picks, and how many the prune keeps (equal: no prune, and a further call continues this one)
    -> (idx int32 (k_keep,), score float32 (k_keep,)) on the device: the kept picks in pick order with their forward scores"""
    import torch
    from . import _abi, net_host
    f, N, F = _table("f", f, torch, blocks)
    dev, m = f.device, int(blocks)
    free = _free_mask(free, N, torch, dev)
    for name, t in (("phi", phi), ("B", B)):
        if not isinstance(t, torch.Tensor) or t.device != dev or t.dtype is not torch.float64 or tuple(t.shape) != (m, F, F) or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 CUDA tensor of shape (%d, %d, %d) on f's device" % (name, m, F, F))
    k_forward, k_keep = int(k_forward), int(k_keep)
    if not 1 <= k_keep <= k_forward <= N:
        raise ValueError("k_forward = %d, k_keep = %d: 1 <= k_keep <= k_forward <= N = %d is needed" % (k_forward, k_keep, N))
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = net_host.aligned_scratch(lib.alink_bait_select_scratch_bytes(N, F, m, k_forward), dev)
    idx = torch.empty(k_keep, dtype=torch.int32, device=dev)
    score = torch.empty(k_keep, dtype=torch.float32, device=dev)
    _abi.check(lib.alink_bait_select(_abi.ptr(f), N, F, m, _abi.ptr(phi), _abi.ptr(B), _abi.ptr(free), k_forward, k_keep,
                                     _abi.ptr(idx), _abi.ptr(score), sp, _abi.current_stream(dev)), "alink_bait_select")
    return idx, score


def bait_factors_device(f, labelled, n_instances, lam=1.0, over=2, blocks=1):
    """A BAIT batch over factor rows resident on the GPU: Phi, the labelled rows' sum and B0 = M0^-1 on the host in float64
    (fisher_matrix over a read-back of the factor rows, N x blocks x F floats: the Gram matrices are not built on the device),
    then bait_select_device.  `labelled`: row indices or None.  -> (idx int32 (k,), score float32 (k,)) on the device, k clipped to the rows not labelled."""
    import torch
    f, N, F = _table("f", f, torch, blocks)
    m = int(blocks)
    if int(n_instances) < 1:
        raise ValueError("n_instances = %r must be at least 1" % (n_instances,))
    if int(over) < 1:
        raise ValueError("over = %r must be at least 1" % (over,))
    lab = _labelled(labelled, N)
    k = min(int(n_instances), N - len(lab))
    if k < 1:
        raise ValueError("bait: every row is labelled")
    dev = f.device
    f64 = f.cpu().numpy().astype(np.float64)               # the one read-back before the loop: the factor rows
    phi = torch.from_numpy(fisher_matrix(f64, scale=1.0 / N, blocks=m)).to(dev)
    M0 = float(lam) * np.eye(F)[None].repeat(m, axis=0) + fisher_matrix(f64, rows=lab, blocks=m)
    free = torch.ones(N, dtype=torch.uint8, device=dev)
    if len(lab):
        free[torch.from_numpy(lab).to(dev)] = 0
    B0 = np.stack([np.linalg.inv(M0[j]) for j in range(m)])
    B0 = 0.5 * (B0 + B0.transpose(0, 2, 1))                # the device reads row k of B for its column k
    B = torch.from_numpy(np.ascontiguousarray(B0)).to(dev)
    return bait_select_device(f, phi, B, free, min(int(over) * k, N - len(lab)), k, blocks=m)


def bait_device(head, L, R, li=None, ri=None, labelled=None, n_instances=1, lam=1.0, over=2):
    """A BAIT batch of the pairs (L[n], R[n]) or (L[li[n]], R[ri[n]]) on the GPU: egl.expected_gradient_length_device's probs and
    emb, fisher_factor_device, bait_factors_device.  EXTENSION.  head: a DenseHead in the float32 compute mode; labelled: indices
    of pairs that are labelled already (they enter M0 and are never picked), or None.  Read back: the factor rows, once, for
    the Gram matrices; the picks stay on the device.  -> (idx int32 (k,), score float32 (k,)) on the device, indices into the pairs."""
    _check_shape(head.h2, 1)
    out = _egl.expected_gradient_length_device(head, L, R, li, ri, want=("probs", "emb"))
    f = fisher_factor_device(out["probs"], out["emb"])
    return bait_factors_device(f, labelled, n_instances, lam=lam, over=over)


def bait_sampling(classifier, X, n_instances=1):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=bait_sampling)): a BAIT batch of n_instances pairs of
    X = [left, right] with nothing labelled (M0 = I).  EXTENSION.  `classifier`: a DenseHead, or a learner / estimator that
    exposes siamese_net.get_weights().  CUDA tensors go through the device route (the head must be a DenseHead: there is no
    fallback), anything else through `bait`.  -> (query_idx, instances): the picks in order; the instances as the other samplers
    of this package return them for pair input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    net = _egl._head_of(classifier)
    on_device = hasattr(X[0], "is_cuda") and X[0].is_cuda
    if on_device:
        if not hasattr(net, "bait_device"):
            raise TypeError("bait_sampling on CUDA tensors needs a DenseHead (got %s)" % type(net).__name__)
        query_idx = net.bait_device(X[0], X[1], n_instances=n_instances)[0].cpu().numpy().astype(np.int64)
        query_idx = query_idx[query_idx >= 0]
        import torch
        take = torch.from_numpy(query_idx).to(X[0].device)
        return query_idx, [X[0][take], X[0][take]]
    query_idx = bait(net.get_weights(), X, None, n_instances)
    return query_idx, [X[0][query_idx], X[0][query_idx]]
