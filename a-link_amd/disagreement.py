"""disagreement — the query-by-committee measures of modAL.disagreement, patched for pair input like uncertainty.py.

The reference imports this module (code/learners.py:12) and names its samplers as Committee's query strategies
(code/learners.py:245, :287).  Measures and samplers have modAL's signatures and are host NumPy / scipy.stats.entropy in
float64 on whatever the committee's `vote` / `vote_proba` / `predict_proba` return (any duck-typed committee with those and
`classes_`, as learners.Committee); `score_members_device` computes the same measures for a pool resident on the GPU, all of
them in one launch (alink_committee_disagreement, select.hip).

    vote entropy        -sum_c (n_c / M) ln(n_c / M) over the members' vote counts n_c
    consensus entropy   entropy of the mean of the members' class probabilities
    max disagreement    max over members of KL(member || consensus)

Kept quirk: the samplers return `[X[0][idx], X[0][idx]]` — the LEFT array twice (code/uncertainty.py:159,187,217).
"""
import numpy as np
from scipy.stats import entropy

from .base import _n
from .learners import vote_entropy_sampling  # noqa: F401  (modAL.disagreement.vote_entropy_sampling: it stays where the reference's import put it)
from .uncertainty import NotFittedError, _pick

DEVICE_OUTPUTS = ("vote_entropy", "consensus_entropy", "max_disagreement", "consensus", "votes")
KINDS = DEVICE_OUTPUTS[:3]


# ---- the formulas on arrays (shared by the measures below and by Bagging's host path) ---------------------------------
def votes_entropy(votes, classes):
    """votes (P, M) class labels, one column per member -> (P,) entropy of the vote distribution over `classes`."""
    votes = np.asarray(votes)
    p_vote = np.stack([(votes == c).sum(axis=1) for c in classes], axis=1) / float(votes.shape[1])
    return entropy(p_vote, axis=1)


def proba_consensus_entropy(member_proba):
    """member_proba (P, M, C) -> (P,) entropy of the members' mean."""
    return entropy(np.mean(np.asarray(member_proba, np.float64), axis=1), axis=1)


def proba_max_disagreement(member_proba):
    """member_proba (P, M, C) -> (P,) max over members of KL(member || mean of the members)."""
    p = np.asarray(member_proba, np.float64)
    consensus = np.mean(p, axis=1)
    kl = np.stack([entropy(p[:, m, :], qk=consensus, axis=1) for m in range(p.shape[1])], axis=1)
    return np.max(kl, axis=1)


# ---- modAL.disagreement measures ------------------------------------------------------------------------------------------
def vote_entropy(committee, X, **predict_kwargs):
    try:
        votes = committee.vote(X, **predict_kwargs)
    except NotFittedError:
        return np.zeros(shape=(_n(X),))
    return votes_entropy(votes, committee.classes_)


def consensus_entropy(committee, X, **predict_proba_kwargs):
    try:
        proba = committee.predict_proba(X, **predict_proba_kwargs)
    except NotFittedError:
        return np.zeros(shape=(_n(X),))
    return np.transpose(entropy(np.transpose(proba)))


def KL_max_disagreement(committee, X, **predict_proba_kwargs):
    try:
        p_vote = committee.vote_proba(X, **predict_proba_kwargs)
    except NotFittedError:
        return np.zeros(shape=(_n(X),))
    return proba_max_disagreement(p_vote)


# ---- modAL.disagreement samplers (vote_entropy_sampling: learners.py) -------------------------------------------------------
def consensus_entropy_sampling(committee, X, n_instances=1, random_tie_break=False, **disagreement_measure_kwargs):
    disagreement = consensus_entropy(committee, X, **disagreement_measure_kwargs)
    query_idx = _pick(disagreement, n_instances, random_tie_break)
    return query_idx, [X[0][query_idx], X[0][query_idx]]


def max_disagreement_sampling(committee, X, n_instances=1, random_tie_break=False, **disagreement_measure_kwargs):
    disagreement = KL_max_disagreement(committee, X, **disagreement_measure_kwargs)
    query_idx = _pick(disagreement, n_instances, random_tie_break)
    return query_idx, [X[0][query_idx], X[0][query_idx]]


# ---- device form: every measure of a pool in one launch ---------------------------------------------------------------------
def score_members_device(member_probs, want=("vote_entropy",)):
    """member_probs: a list of M CUDA (P, C) float32 tensors, or one (M, P, C) tensor (head.committee_member_probs_device)
    -> {name: CUDA tensor} for the names in `want`, among vote_entropy / consensus_entropy / max_disagreement (P,),
    consensus (P, C) float32 and votes (P, M) int32 (each member's argmax class).  consensus is bit-equal to
    head.committee_predict_device of the same members, consensus_entropy to uncertainty.score_device(consensus, "entropy");
    equal vote counts in any class order give bit-equal vote_entropy, so uncertainty.topk_device breaks its many ties by
    the lower index (include/alink_hip.h)."""
    import ctypes as C
    import torch
    from . import _abi
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in DEVICE_OUTPUTS]
    if unknown:
        raise ValueError("unknown disagreement output(s) %s: choose among %s" % (unknown, list(DEVICE_OUTPUTS)))
    if isinstance(member_probs, torch.Tensor):
        if member_probs.dim() != 3:
            raise ValueError("member_probs: one (M, P, C) tensor or a list of (P, C) tensors")
        member_probs = list(member_probs.unbind(0))
    members = [p.to(torch.float32).contiguous() for p in member_probs]
    if not members or not members[0].is_cuda or members[0].dim() != 2:
        raise ValueError("member_probs: at least one CUDA (P, C) tensor")
    if any(p.shape != members[0].shape or p.device != members[0].device for p in members):
        raise ValueError("every member's probabilities must have one shape and one device")
    dev = members[0].device
    lib = _abi.init(dev.index or 0)
    M = len(members)
    P, Cn = members[0].shape
    shapes = {"consensus": ((P, Cn), torch.float32), "votes": ((P, M), torch.int32)}
    out = {}
    for w in want:
        shape, dtype = shapes.get(w, ((P,), torch.float32))
        out[w] = torch.empty(shape, dtype=dtype, device=dev)
    arr = (C.c_void_p * M)(*[p.data_ptr() for p in members])
    _abi.check(lib.alink_committee_disagreement(arr, M, P, Cn, *[_abi.ptr(out.get(w)) for w in DEVICE_OUTPUTS],
                                                _abi.current_stream(dev)), "alink_committee_disagreement")
    return out
