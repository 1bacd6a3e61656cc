"""egl — expected gradient length (Settles, Craven & Ray 2008) and the last layer's gradient embedding (BADGE: Ash et al.
2020) of the pair scorer.  EXTENSION: the reference imports its strategies from modAL, and every one of them
scores a pair from the head's output probabilities alone; no reference driver names this one.

Two pairs with the same P(same) can move the weights by very different amounts.  The expected gradient length asks how far
the fine-tune step would move the scorer if this pair were labelled, averaged over the labels the scorer itself expects.  For
one pair x let l_c(x) be the loss the train step computes on the batch {x} with target class c and sample weight 1 (Keras'
binary_crossentropy on the head's output: p clipped to [1e-7, 1 - 1e-7], mean over the outputs) and g_c(x) its gradient over
all six parameter tensors:

    EGL(x) = sum over c in {0, 1} of P(c | x) |g_c(x)|_2          P(c | x) = the head's probability; one output: p, 1 - p

The per-sample gradient of a dense layer is rank one, so no weight gradient is formed.  With d = |l - r|, a1 = relu(z1),
a2 = relu(z2) and dz3 = p - y for both head types:

    u   = (W3[:,0] - W3[:,1]) . [z2 > 0], n3 = 2        one output: u = W3[:,0] . [z2 > 0], n3 = 1
    v   = (u W2^T) . [z1 > 0]
    G^2 = n3 (|a2|^2 + 1) + |u|^2 (|a1|^2 + 1) + |v|^2 (|d|^2 + 1)
    EGL = 2 p0 p1 sqrt(G^2)                             one output: 2 p (1 - p) sqrt(G^2)

A row with an output outside [1e-7, 1 - 1e-7] has EGL exactly 0: the clip kills the step's gradient there, and that is the
train step's behaviour, kept on purpose.  The gradient embedding of a row is the last layer's weight gradient for the label
the scorer itself would give, yhat = argmax p (ties to class 0; one output: p > 0.5):

    emb[n, c h2 + j] = (p_c - [c = yhat]) a2[j]         zero on a saturated row, like the step's gradient

`expected_gradient_length`, `gradient_embedding` are host float64 NumPy; `egl_sampling` is modAL-shaped;
`expected_gradient_length_device` is the form for a pool resident on the GPU (alink_head_egl, egl.hip: one forward pass plus
one h2 -> h1 back-projection per pair, in one launch).  BADGE's k-means++ sampling over the embeddings is badge.py (X10).  Not
on the device: a bf16-mode form, several ranks' pools in one call.
"""
import numpy as np

from .batch import _f32_matrix
from .uncertainty import multi_argmax

DEVICE_OUTPUTS = ("egl", "probs", "emb")
_CLIP = 1e-7


def _host_pass(weights, X):
    """float64 forward of the head -> (p (N, od), d, a1, z1, a2, z2, W2, W3)"""
    if len(weights) != 6:
        raise ValueError("weights: the Keras-ordered list [W1, b1, W2, b2, W3, b3] is needed (got %d arrays)" % len(weights))
    W1, b1, W2, b2, W3, b3 = [np.asarray(w, np.float64) for w in weights]
    d = np.abs(np.asarray(X[0], np.float64) - np.asarray(X[1], np.float64))
    z1 = d @ W1 + b1
    a1 = np.maximum(z1, 0)
    z2 = a1 @ W2 + b2
    a2 = np.maximum(z2, 0)
    z3 = a2 @ W3 + b3
    if z3.shape[1] > 1:
        e = np.exp(z3 - z3.max(axis=1, keepdims=True))
        p = e / e.sum(axis=1, keepdims=True)
    else:
        with np.errstate(over="ignore"):                  # exp(-z) = inf gives p = 0: a saturated row
            p = 1 / (1 + np.exp(-z3))
    return p, d, a1, z1, a2, z2, W2, W3


def _inside(p):
    """rows whose every output lies in the loss's clip range"""
    return ((p >= _CLIP) & (p <= 1 - _CLIP)).all(axis=1)


def expected_gradient_length(weights, X):
    """EGL of every pair of X = [left, right] under the head `weights` = [W1, b1, W2, b2, W3, b3] (Keras order; W3 with two
    columns: softmax, with one: sigmoid).  EXTENSION.  -> (N,) float64, the closed form of the module docstring."""
    p, d, a1, z1, a2, z2, W2, W3 = _host_pass(weights, X)
    od = p.shape[1]
    wd = W3[:, 0] - W3[:, 1] if od == 2 else W3[:, 0]
    u = wd[None, :] * (z2 > 0)
    v = (u @ W2.T) * (z1 > 0)
    sq = lambda a: (a * a).sum(axis=1)
    g2 = od * (sq(a2) + 1) + sq(u) * (sq(a1) + 1) + sq(v) * (sq(d) + 1)
    pq = p[:, 0] * p[:, 1] if od == 2 else p[:, 0] * (1 - p[:, 0])
    return np.where(_inside(p), 2 * pq * np.sqrt(g2), 0.0)


def gradient_embedding(weights, X):
    """The gradient embedding of every pair of X = [left, right]: the last layer's weight gradient for the label the head itself
    would give.  EXTENSION.  -> (N, od * h2) float64, emb[n, c * h2 + j] = (p_c - [c = yhat]) a2[j]; zero on a saturated row."""
    p, _, _, _, a2, _, _, _ = _host_pass(weights, X)
    od = p.shape[1]
    hit = np.zeros_like(p)
    if od == 2:
        hit[np.arange(len(p)), (p[:, 1] > p[:, 0]).astype(int)] = 1.0
    else:
        hit[:, 0] = p[:, 0] > 0.5
    dz = np.where(_inside(p)[:, None], p - hit, 0.0)
    return (dz[:, :, None] * a2[:, None, :]).reshape(len(p), od * a2.shape[1])


def _head_of(classifier):
    """the object with get_weights(): the classifier itself (a DenseHead), its siamese_net, or its estimator's"""
    for obj in (classifier, getattr(classifier, "estimator", None)):
        if obj is None:
            continue
        net = getattr(obj, "siamese_net", obj)
        if hasattr(net, "get_weights"):
            return net
    raise TypeError("egl_sampling needs the scorer's weights: a DenseHead, or a classifier whose estimator exposes siamese_net.get_weights()")


def egl_sampling(classifier, X, n_instances=1):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=egl_sampling)): the n_instances pairs of X = [left, right] with
    the largest expected gradient length.  EXTENSION.  `classifier`: a DenseHead, or a learner / estimator that exposes
    siamese_net.get_weights().  CUDA tensors are scored on the device (the head must be a DenseHead: there is no fallback),
    anything else on the host.  -> (query_idx, instances): ties as uncertainty.multi_argmax breaks them; the instances as the
    other samplers of this package return them for pair input, `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    net = _head_of(classifier)
    on_device = hasattr(X[0], "is_cuda") and X[0].is_cuda
    if on_device:
        if not hasattr(net, "expected_gradient_length_device"):
            raise TypeError("egl_sampling on CUDA tensors needs a DenseHead (got %s)" % type(net).__name__)
        values = net.expected_gradient_length_device(X[0], X[1])["egl"].cpu().numpy()
    else:
        values = expected_gradient_length(net.get_weights(), X)
    query_idx = multi_argmax(values, n_instances=n_instances)
    if on_device:
        import torch
        take = torch.from_numpy(np.asarray(query_idx, np.int64)).to(X[0].device)
        return query_idx, [X[0][take], X[0][take]]
    if isinstance(X, (list, tuple)):
        return query_idx, [X[0][query_idx], X[0][query_idx]]
    return query_idx, X[query_idx]


# ---- device form: one launch for the pool, pairs gathered by index from the two feature tables ----------------------------
def _index_vector(name, v, table, torch, dev):
    if not isinstance(v, torch.Tensor) or not v.is_cuda or v.device != dev:
        raise ValueError("%s must be a CUDA tensor on the head's device" % name)
    if v.dtype is not torch.int32 or v.dim() != 1:
        raise ValueError("%s must be a 1-D int32 tensor (got %s, shape %s)" % (name, v.dtype, tuple(v.shape)))
    if v.numel() and (int(v.min()) < 0 or int(v.max()) >= table.shape[0]):
        raise ValueError("%s points outside its table of %d rows" % (name, table.shape[0]))
    return v.contiguous()


def expected_gradient_length_device(head, L, R, li=None, ri=None, want=("egl",), egl_out=None, accumulate=False, final_div=0.0):
    """EGL, probabilities and gradient embeddings of a pool on the GPU (alink_head_egl).  EXTENSION.

    head    a DenseHead in the float32 compute mode
    L, R    CUDA float32 (., D) feature tables on the head's device; without li / ri pair n is (L[n], R[n]), with them
            (L[li[n]], R[ri[n]]) — int32 (P,) index vectors, range-checked here, the pairs never materialised
    want    names among egl (P,), probs (P, od): DenseHead.predict_device's bits, emb (P, od * h2)
    egl_out, accumulate, final_div   the committee mean (Bagging.egl_indexed): write egl into egl_out, adding to what is there,
            and divide by final_div (> 0) after adding
    -> {name: CUDA float32 tensor}.  Nothing is synchronised or read back except the range check of li / ri."""
    from . import _abi
    torch = head.torch
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in DEVICE_OUTPUTS]
    if unknown or not want:
        raise ValueError("unknown egl output(s) %s: choose among %s" % (unknown, list(DEVICE_OUTPUTS)))
    dev = head._tdev
    L = _f32_matrix("L", L, torch, dev)
    if L.shape[1] != head.d_in:
        raise ValueError("L has D = %d, the head D = %d" % (L.shape[1], head.d_in))
    R = _f32_matrix("R", R, torch, dev, head.d_in)
    if (li is None) != (ri is None):
        raise ValueError("li and ri come together: both index vectors, or neither")
    if li is not None:
        li, ri = _index_vector("li", li, L, torch, dev), _index_vector("ri", ri, R, torch, dev)
        if li.numel() != ri.numel():
            raise ValueError("li and ri differ in length (%d, %d)" % (li.numel(), ri.numel()))
        P = li.numel()
    else:
        if L.shape[0] != R.shape[0]:
            raise ValueError("L and R differ in rows (%d, %d): without li / ri pair n is (L[n], R[n])" % (L.shape[0], R.shape[0]))
        P = L.shape[0]
    if head.compute_dtype != "f32":
        raise ValueError("expected_gradient_length_device is the exact float32 form: the head is in the %s compute mode" % head.compute_dtype)
    shapes = {"egl": (P,), "probs": (P, head.out_dim), "emb": (P, head.out_dim * head.h2)}
    out = {w: torch.empty(shapes[w], dtype=torch.float32, device=dev) for w in want}
    if egl_out is not None:
        if "egl" not in out or egl_out.shape != shapes["egl"] or egl_out.dtype is not torch.float32 or egl_out.device != dev or not egl_out.is_contiguous():
            raise ValueError("egl_out: a contiguous float32 (%d,) tensor on the head's device, with \"egl\" among the outputs" % P)
        out["egl"] = egl_out
    if P:
        _abi.check(head.lib.alink_head_egl(head.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(li), _abi.ptr(ri), P, int(bool(accumulate)),
                                           float(final_div), *[_abi.ptr(out.get(w)) for w in DEVICE_OUTPUTS],
                                           _abi.current_stream(head.device)), "alink_head_egl")
    return out
