"""facility — facility-location batches: the k rows that best REPRESENT a pool, by the greedy of largest gain, plain or stochastic.
EXTENSION: the reference imports its strategies from modAL, which has no such sampler; no reference driver
names these.

Facility location asks for the k rows S that minimise L(S) = sum_n min_(s in S) |x_n - x_s|^2: the graded form of what ProbCover
(probcover.py) asks with a 0/1 objective.  It is the selection rule of FASS (Wei, Iyer & Bilmes 2015, "Submodularity in Data
Subset Selection and Active Learning": filter to the beta * k most uncertain rows, then facility location among them), of CRAIG's
coresets and of the SIMILAR family.  L is supermodular and its greedy carries the (1 - 1/e) guarantee; the stochastic greedy of
Mirzasoleiman et al. 2015 ("Lazier Than Lazy Greedy") takes each pick among a random sample of R ~ (N / k) ln(1 / eps)
candidates instead of all N and keeps (1 - 1/e - eps) in expectation.

The rule (include/alink_hip.h, alink_facility_gains, states it in full):

    score   t(n, j) = |x_n|^2 + |x_j|^2 - 2 x_n . x_j, ProbCover's;  w(n, j) = 0 if t < 0, else t (a NaN stays).  No self-exemption.
    term    term(n, c) = d if d > 0, else 0, with d = cur_n - w(n, c); a NaN on either side gives 0; a row whose squared norm is not
            finite in float32 gives 0.  `cur` (N,) float32 is the caller's: each row's squared distance to its nearest facility.
    gain    gain(c) = sum_n term(n, c) in float64.  A candidate index outside 0 .. N - 1, or with a non-finite norm, has gain 0.
    pick    the candidate POSITION of largest gain wins by `>` from 0, ties to the lower position in the candidate list;
            pick = cand[position].  If no gain is > 0: the pick is -1 with gain 0, cur is unchanged, later steps go on.
    cover   cur_n <- w(n, s) where w(n, s) < cur_n, for every s of an index list; an s outside 0 .. N - 1 (or -1), or with a
            non-finite norm, is ignored.  After a pick p, cur_p <= w(p, p): p's gain is exactly 0 in every later step, and a
            labelled row, covered before the first pick, is never picked either.

`gains`, `cover`, `select` and `facility` are that rule in host float64 NumPy from the float32 rows (an N x R matrix per pick:
small pools only); the `_device` forms are alink_facility_gains, alink_facility_cover and alink_facility_select (facility.hip:
the N x R scores on the matrix cores, never in memory; three launches per pick, nothing read back).  On the device w is float32
in the order of ProbCover's t; where nothing rounds, as on small-integer rows with an integer cur, host and device agree bit
for bit.

`sample_candidates` draws each step's candidates WITH replacement, which departs from the paper (it samples without): a
duplicate ties with its first occurrence, which wins as the lower position, and a row already picked has gain 0, so neither
changes what a step can pick — they only make the effective sample a little smaller than R.

Not built: lazy-greedy bounds, row weights, a cosine metric, the cover of pick t fused into the gains pass of pick t + 1, several
ranks' pools in one call.
"""
import numpy as np

from . import cluster as _cluster
from .batch import _rows
from .typiclust import _labelled_indices
from .uncertainty import classifier_uncertainty


def _host_rows(rows):
    """-> (X float64 (N, D) from the float32 rows, norms float64 (N,), alive bool (N,): the float32 norm is finite)"""
    X = np.asarray(rows, np.float32).astype(np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("rows: a non-empty (N, D) array is needed (got shape %s)" % (X.shape,))
    with np.errstate(invalid="ignore", over="ignore"):
        norms = (X * X).sum(axis=1)
        alive = np.isfinite(norms.astype(np.float32))
    return X, norms, alive


def _host_cur(cur, N):
    c = np.asarray(cur, np.float32).reshape(-1)
    if c.shape != (N,):
        raise ValueError("cur: %d values are needed (got %d)" % (N, c.size))
    return c


def _w_columns(X, norms, alive, cols):
    """w(n, c) float64 (N, len(cols)) for the alive rows `cols`; rows that are not alive come back as NaN"""
    with np.errstate(invalid="ignore", over="ignore"):
        Xa = np.where(alive[:, None], X, 0.0)
        t = (norms[:, None] + norms[cols][None, :]) - 2.0 * (Xa @ Xa[cols].T)
        w = np.where(t < 0, 0.0, t)
    w[~alive] = np.nan
    return w


def _check_k(k):
    if int(k) != k or int(k) < 1:
        raise ValueError("k = %r must be an integer >= 1" % (k,))
    return int(k)


def _gains(X, norms, alive, cur, cand):
    N = len(X)
    ok = (cand >= 0) & (cand < N)
    ok[ok] = alive[cand[ok]]
    out = np.zeros(len(cand), np.float64)
    if ok.any():
        w = _w_columns(X, norms, alive, cand[ok])
        with np.errstate(invalid="ignore"):
            d = cur.astype(np.float64)[:, None] - w
            out[ok] = np.where(d > 0, d, 0.0).sum(axis=0)          # (a NaN on either side: d > 0 is False)
    return out


def _cover(X, norms, alive, cur, sel):
    N = len(X)
    sel = sel[(sel >= 0) & (sel < N)]
    sel = sel[alive[sel]]
    for s0 in range(0, len(sel), 256):
        w = _w_columns(X, norms, alive, sel[s0:s0 + 256])
        with np.errstate(invalid="ignore"):
            best = np.fmin.reduce(w, axis=1)                       # (rows that are not alive: NaN, never `<`)
            less = best < cur.astype(np.float64)
        cur[less] = best[less].astype(np.float32)
    return cur


def _candidate_list(cand, N, what, k=None):
    if cand is None:
        return None
    c = np.asarray(cand)
    if c.dtype.kind not in "iu" or c.ndim != (1 if k is None else 2) or (k is not None and c.shape[0] != k) or c.shape[-1] < 1:
        raise ValueError("%s: None, or integers of shape %s are needed (got %s, shape %s)"
                         % (what, "(R,)" if k is None else "(%d, R)" % k, c.dtype, c.shape))
    if c.shape[-1] > N:
        raise ValueError("%s: R = %d candidates for a pool of %d rows" % (what, c.shape[-1], N))
    return c.astype(np.int64)


def gains(rows, cur, cand=None):
    """gain(c) of every candidate on the host, the rule of the module docstring.  EXTENSION.
    cand: None (every row: position r = row r) or R <= N integers.  -> float64 (R,)."""
    X, norms, alive = _host_rows(rows)
    c = _candidate_list(cand, len(X), "cand")
    return _gains(X, norms, alive, _host_cur(cur, len(X)), np.arange(len(X)) if c is None else c)


def cover(rows, cur, sel):
    """cur after covering with the rows `sel` (integers; outside 0 .. N - 1: ignored) on the host.  EXTENSION.
    -> float32 (N,), a new array."""
    X, norms, alive = _host_rows(rows)
    return _cover(X, norms, alive, _host_cur(cur, len(X)).copy(), np.asarray(sel, np.int64).reshape(-1))


def select(rows, cur, k, cand=None):
    """k greedy picks on the host.  EXTENSION.  cand: None (every row at every step) or (k, R) integers, one list per step.
    -> (picks int32 (k,), gain float64 (k,), cur float32 (N,) after the last pick — a new array)."""
    X, norms, alive = _host_rows(rows)
    N, k = len(X), _check_k(k)
    c = _candidate_list(cand, N, "cand", k)
    cur = _host_cur(cur, N).copy()
    picks, gain = np.full(k, -1, np.int32), np.zeros(k, np.float64)
    every = np.arange(N)
    for t in range(k):
        ct = every if c is None else c[t]
        g = _gains(X, norms, alive, cur, ct)
        pos = int(np.argmax(g))                                    # the first of equal maxima: ties to the lower position
        if not g[pos] > 0:
            continue
        picks[t], gain[t] = ct[pos], g[pos]
        _cover(X, norms, alive, cur, ct[pos:pos + 1])
    return picks, gain, cur


def default_cap(rows):
    """4 max |x_n|^2 over the rows of finite norm, as float32: no squared distance between two rows exceeds it
    (|a - b|^2 <= 2 |a|^2 + 2 |b|^2).  ValueError when no row has a finite norm."""
    _, norms, alive = _host_rows(rows)
    return _cap_of(norms[alive].astype(np.float32))


def _cap_of(finite_norms):
    if finite_norms.size == 0:
        raise ValueError("default_cap: no row has a finite norm")
    with np.errstate(over="ignore"):
        cap = np.float32(4.0) * np.float32(finite_norms.max())
    if not np.isfinite(cap):
        raise ValueError("default_cap: 4 max |x|^2 is not finite in float32")
    return cap


def n_candidates(N, k, eps=0.01):
    """R = min(N, ceil(N / k ln(1 / eps))), the sample size of the stochastic greedy"""
    if not 0.0 < float(eps) < 1.0:
        raise ValueError("eps = %r outside (0, 1)" % (eps,))
    return int(max(1, min(N, int(np.ceil(float(N) / _check_k(k) * np.log(1.0 / float(eps)))))))


def sample_candidates(N, k, eps=0.01, random_state=None):
    """The stochastic greedy's candidates: np.random.RandomState(random_state).randint(0, N, (k, R)), R = n_candidates(N, k, eps),
    as int32 — WITH replacement (the module docstring says why that is harmless)."""
    R = n_candidates(N, k, eps)
    return np.random.RandomState(random_state).randint(0, N, (k, R)).astype(np.int32)


def _plan(N, labelled, n_instances, fill):
    n = _cluster._check_instances(n_instances)
    lab = _labelled_indices(labelled, N)
    if fill not in (None, "random"):
        raise ValueError("fill = %r: None or 'random'" % (fill,))
    return lab, min(n, N - len(lab))


def _cap(cap, finite_norms):
    if cap is None:
        return _cap_of(finite_norms)
    c = np.float32(cap)
    if not (np.isfinite(c) and c > 0):
        raise ValueError("cap = %r: it must be finite and > 0 in float32" % (cap,))
    return c


def _finish(picks, gain, cur, alive, lab, n, fill, random_state, cap):
    """the greedy picks, the random fill and the info dict, the same on both routes (host arrays) — probcover._finish's pattern"""
    real = picks[picks >= 0].astype(np.int64)
    exhausted = len(real) < n
    out = real
    if exhausted and fill == "random":
        free = alive.copy()
        free[lab] = False
        free[real] = False
        rest = np.flatnonzero(free)
        take = min(n - len(real), len(rest))
        if take:
            out = np.concatenate([real, np.random.RandomState(random_state).choice(rest, take, replace=False).astype(np.int64)])
    with np.errstate(invalid="ignore"):
        objective = float(np.nansum(cur[alive].astype(np.float64)))
    info = {"cap": float(cap), "gain": gain[picks >= 0].astype(np.float64), "objective": objective, "exhausted": bool(exhausted)}
    return out, info


def facility(rows, labelled, n_instances, cap=None, eps=None, fill=None, random_state=None):
    """Facility-location queries on the host: n_instances picks among the rows of the (N, D) array `rows`.  EXTENSION.

    labelled      row indices into `rows` (ProbCover's convention): covered before the first pick, so never picked
    n_instances   clipped to the rows that are not labelled
    cap           cur starts at this float32 everywhere; None: default_cap(rows)
    eps           None: the plain greedy, every row a candidate at every step; a number in (0, 1): the stochastic greedy over
                  sample_candidates(N, n, eps, random_state)
    fill          None: a step without a gain (-1) is dropped; "random": the batch is filled to n with rows drawn uniformly,
                  without replacement, from the rows of finite norm neither labelled nor picked (np.random.RandomState(random_state))
    -> (picks int64, info): info holds "cap", "gain" (per greedy pick), "objective" (sum of cur after the last pick) and
    "exhausted" (fewer than n greedy picks)."""
    X, norms, alive = _host_rows(rows)
    N = len(X)
    lab, n = _plan(N, labelled, n_instances, fill)
    cap = _cap(cap, norms[alive].astype(np.float32))
    cur = np.full(N, cap, np.float32)
    if n < 1:
        return np.zeros(0, np.int64), {"cap": float(cap), "gain": np.zeros(0), "objective": float("nan"), "exhausted": False}
    _cover(X, norms, alive, cur, lab)
    cand = None if eps is None else sample_candidates(N, n, eps, random_state)
    picks, gain, cur = select(rows, cur, n, cand)
    return _finish(picks, gain, cur, alive, lab, n, fill, random_state, cap)


# ---- device forms -------------------------------------------------------------------------------------------------------------
def _pool(rows, what):
    from .probcover import _pool as _pb_pool
    pool, N, D, dev, _ = _pb_pool(rows, None, what)
    return pool, N, D, dev


def _cur_vector(cur, N, dev, torch):
    if not isinstance(cur, torch.Tensor) or cur.device != dev or cur.dtype is not torch.float32 or cur.shape != (N,):
        raise ValueError("cur: a float32 tensor of %d values on the pool's device is needed" % N)
    return cur.contiguous()


def _index_tensor(v, what, dev, torch, shape_of=None):
    """None, host integers or an int32 tensor on the pool's device -> contiguous int32 tensor (or None)"""
    if v is None:
        return None
    if not isinstance(v, torch.Tensor):
        a = np.asarray(v)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("%s: integers are needed (got %s)" % (what, a.dtype))
        v = torch.from_numpy(a.astype(np.int32)).to(dev)
    if v.device != dev or v.dtype is not torch.int32:
        raise ValueError("%s: an int32 tensor on the pool's device is needed" % what)
    return v.contiguous()


def _scratch(lib, N, D, R, k, dev):
    from . import net_host
    return net_host.aligned_scratch(lib.alink_facility_scratch_bytes(N, D, R, k), dev)


def gains_device(rows, cur, cand=None):
    """gain(c) of every candidate on the GPU (alink_facility_gains).  EXTENSION.

    rows  the pool as in cluster.kmeans_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri)
    cur   CUDA float32 (N,)
    cand  None (every row: position r = row r), or R <= N integers (host, or a CUDA int32 tensor)
    -> float64 (R,) on the device.  Nothing is synchronised or read back."""
    import torch
    from . import _abi
    (left, right, li, ri), N, D, dev = _pool(rows, "gains_device")
    cur = _cur_vector(cur, N, dev, torch)
    cand = _index_tensor(cand, "cand", dev, torch)
    if cand is not None and (cand.dim() != 1 or not 1 <= cand.numel() <= N):
        raise ValueError("cand: 1 .. %d candidates in a 1-D list are needed" % N)
    R = N if cand is None else cand.numel()
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = _scratch(lib, N, D, R, 1, dev)
    gain = torch.empty(R, dtype=torch.float64, device=dev)
    _abi.check(lib.alink_facility_gains(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(cur), _abi.ptr(cand),
                                        R, _abi.ptr(gain), sp, _abi.current_stream(dev)), "alink_facility_gains")
    return gain


def cover_device(rows, cur, sel):
    """cur after covering with the rows `sel` on the GPU (alink_facility_cover).  EXTENSION.  rows, cur as in gains_device; sel:
    integers (host, or a CUDA int32 tensor), those outside 0 .. N - 1 ignored.  -> float32 (N,) on the device, a new tensor."""
    import torch
    from . import _abi
    (left, right, li, ri), N, D, dev = _pool(rows, "cover_device")
    cur = _cur_vector(cur, N, dev, torch).clone()
    sel = _index_tensor(sel, "sel", dev, torch)
    S = 0 if sel is None else sel.numel()
    if S == 0:
        return cur
    if sel.dim() != 1:
        raise ValueError("sel: a 1-D list is needed")
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = _scratch(lib, N, D, 1, 1, dev)
    _abi.check(lib.alink_facility_cover(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(cur), _abi.ptr(sel), S,
                                        sp, _abi.current_stream(dev)), "alink_facility_cover")
    return cur


def select_device(rows, cur, k, cand=None):
    """k greedy picks on the GPU (alink_facility_select): three launches per pick, all enqueued at once.  EXTENSION.  rows, cur as
    in gains_device; cand: None (every row at every step) or (k, R) integers (host, or a CUDA int32 tensor), one list per step.
    -> (picks int32 (k,), gain float64 (k,), cur float32 (N,) after the last pick — a new tensor) on the device.  Nothing is
    synchronised or read back."""
    import torch
    from . import _abi
    (left, right, li, ri), N, D, dev = _pool(rows, "select_device")
    cur = _cur_vector(cur, N, dev, torch).clone()
    k = _check_k(k)
    cand = _index_tensor(cand, "cand", dev, torch)
    if cand is not None and (cand.dim() != 2 or cand.shape[0] != k or not 1 <= cand.shape[1] <= N):
        raise ValueError("cand: (%d, R) candidates with R in 1 .. %d are needed" % (k, N))
    R = N if cand is None else cand.shape[1]
    lib = _abi.init(dev.index or 0)
    scratch, sp, _ = _scratch(lib, N, D, R, k, dev)
    picks = torch.empty(k, dtype=torch.int32, device=dev)
    gain = torch.empty(k, dtype=torch.float64, device=dev)
    _abi.check(lib.alink_facility_select(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(cur), _abi.ptr(cand),
                                         R, k, _abi.ptr(picks), _abi.ptr(gain), sp, _abi.current_stream(dev)), "alink_facility_select")
    return picks, gain, cur


def _norms_device(pool, N, torch):
    """|x_n|^2 as float32 from float64 sums of the float32 rows (the host's), in chunks"""
    left, right, li, ri = pool
    out = torch.empty(N, dtype=torch.float32, device=left.device)
    for n0 in range(0, N, 65536):
        n1 = min(N, n0 + 65536)
        x = left[n0:n1] if li is None else (left.index_select(0, li[n0:n1].long()) - right.index_select(0, ri[n0:n1].long())).abs()
        out[n0:n1] = (x.double() ** 2).sum(dim=1).float()
    return out


def facility_device(rows, labelled, n_instances, cap=None, eps=None, fill=None, random_state=None):
    """Facility-location queries on the GPU: cover_device with the labelled rows, then select_device.  EXTENSION.

    rows      the pool as in gains_device; labelled: host integers, row indices into it
    the rest as in facility.  -> (picks int64 NumPy array, info), facility's; info["cur"] is the device tensor after the last
    pick.  Read back: with cap=None the largest finite norm, and at the end picks, gains, cur and the N-byte finite-norm flags."""
    import torch
    pool, N, D, dev = _pool(rows, "facility_device")
    lab, n = _plan(N, labelled, n_instances, fill)
    norms = _norms_device(pool, N, torch)
    alive_t = torch.isfinite(norms)
    cap = _cap(cap, norms[alive_t].max().reshape(1).cpu().numpy() if bool(alive_t.any()) else np.zeros(0, np.float32))
    cur = torch.full((N,), float(cap), dtype=torch.float32, device=dev)
    if n < 1:
        return np.zeros(0, np.int64), {"cap": float(cap), "gain": np.zeros(0), "objective": float("nan"), "exhausted": False,
                                       "cur": cur}
    if len(lab):
        cur = cover_device(rows, cur, lab)
    cand = None if eps is None else sample_candidates(N, n, eps, random_state)
    picks, gain, cur = select_device(rows, cur, n, cand)
    out, info = _finish(picks.cpu().numpy(), gain.cpu().numpy(), cur.cpu().numpy(), alive_t.cpu().numpy(), lab, n, fill, random_state,
                        cap)
    info["cur"] = cur
    return out, info


def _check_beta(beta):
    if beta is not None and (int(beta) != beta or int(beta) < 1):
        raise ValueError("beta = %r must be None or an integer >= 1" % (beta,))


def facility_sampling(classifier, X, n_instances=1, beta=10, eps=None, cap=None, random_state=None, **uncertainty_measure_kwargs):
    """modAL-shaped query strategy (ActiveLearner(query_strategy=facility_sampling)): FASS (Wei, Iyer & Bilmes 2015) — keep the
    beta * k rows of largest classification uncertainty (uncertainty.classifier_uncertainty; ties to the lower index; beta=None
    keeps the whole pool and does not consult the classifier) and query the k rows that best represent them: facility location,
    plain (eps=None) or stochastic.  EXTENSION.  X is an (N, D) array or pair input [left, right] (rows |left - right|).  A step
    without a gain (duplicate rows) is filled at random, so a call returns min(n_instances, N) rows.  CUDA tensors go through
    facility_device, anything else through facility.  random_state: the seed of the candidate samples and of the fill.
    -> (query_idx, instances): the instances as the other samplers of this package return them for pair input,
    `[X[0][idx], X[0][idx]]` (uncertainty.py's kept quirk)."""
    k = _cluster._check_instances(n_instances)
    _check_beta(beta)
    on_device = _cluster._is_cuda(X)
    utility = None if beta is None else classifier_uncertainty(classifier, X, **uncertainty_measure_kwargs)
    if on_device:
        import torch
        from . import uncertainty as _unc
        rows = (X[0] - X[1]).abs() if isinstance(X, (list, tuple)) else X
        N = rows.shape[0]
        k = min(k, N)
        top = None
        if utility is not None and int(beta) * k < N:
            u = torch.as_tensor(np.asarray(utility.cpu() if hasattr(utility, "cpu") else utility, np.float32)).to(rows.device)
            if u.shape != (N,):
                raise ValueError("the classifier's uncertainty has shape %s for %d rows" % (tuple(u.shape), N))
            top = _unc.topk_device(u, int(beta) * k)[0].long()
            rows = rows.index_select(0, top)
        query_idx, _ = facility_device(rows.to(torch.float32), None, k, cap=cap, eps=eps, fill="random", random_state=random_state)
        if top is not None:
            query_idx = top.cpu().numpy()[query_idx]
    else:
        rows = _rows(X)
        N = len(rows)
        k = min(k, N)
        top = None
        if utility is not None and int(beta) * k < N:
            u = np.asarray(utility, np.float32)
            if u.shape != (N,):
                raise ValueError("the classifier's uncertainty has shape %s for %d rows" % (u.shape, N))
            top = np.argsort(-u, kind="stable")[:int(beta) * k]                # the largest, ties to the lower index
            rows = rows[top]
        query_idx, _ = facility(rows, None, k, cap=cap, eps=eps, fill="random", random_state=random_state)
        if top is not None:
            query_idx = top[query_idx]
    query_idx = np.asarray(query_idx, np.int64)
    return query_idx, _cluster._instances(X, query_idx, on_device)
