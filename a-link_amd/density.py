"""density — information density of modAL.density (Settles & Craven 2008), patched for pair input like batch.py.  EXTENSION
(DESIGN.md §0, X8): the reference imports its strategies from modAL; no reference driver names this one.

A top-k sampler spends its batch on outliers as readily as on near-duplicates: a row far from everything is uncertain and
teaches little about the rest.  Information density measures how representative a row is,

    density_n = mean over j of 1 / (1 + dist(x_n, x_j))                   self-pairs count (dist = 0, similarity = 1)

and density weighting ranks on utility x density^beta (`density_weighted`): the other standard answer, beside batch.py's
ranked batch, to what a plain top-k does with its batch.

`similarize_distance`, `cosine_similarity`, `euclidean_similarity` and `information_density` have modAL's signatures and are
host float64 NumPy + scipy / sklearn, any sklearn metric; `information_density` builds the full N x N matrix, as modAL does.
`information_density_device` is the Euclidean form for a pool resident on the GPU (alink_information_density, density.hip):
nothing N x N is ever stored, the reference set may be smaller than the pool (a random sample, the gallery), and the same pass
gives the mean distance of every row and the row with the least — the cold start of batch.ranked_batch_cold_device.  Not on
the device: other metrics, several ranks' pools in one call.

A pair input X = [left, right] is represented by the rows |left - right| (batch._rows), which is what the pair scorer itself
sees (code/siamese.py:27-35).
"""
import numpy as np

from .batch import _f32_matrix, _pool_rows, _rows

DEVICE_OUTPUTS = ("density", "mean_distance", "central")


def similarize_distance(distance_measure):
    """modAL.density.similarize_distance: a distance -> the similarity 1 / (1 + distance)."""
    def sim(*args, **kwargs):
        return 1 / (1 + distance_measure(*args, **kwargs))
    return sim


def _scipy(name):
    def distance(*args, **kwargs):
        from scipy.spatial import distance as D
        return getattr(D, name)(*args, **kwargs)
    distance.__name__ = name
    return distance


cosine_similarity = similarize_distance(_scipy("cosine"))
euclidean_similarity = similarize_distance(_scipy("euclidean"))


def information_density(X, metric='euclidean'):
    """modAL.density.information_density: (N,) float64, the mean similarity of every row to all rows (itself included)."""
    from sklearn.metrics.pairwise import pairwise_distances
    X = _rows(X)
    similarity_mtx = 1 / (1 + pairwise_distances(X, X, metric=metric))
    return similarity_mtx.mean(axis=1)


def density_weighted(utility, density, beta=1.0):
    """utility x density^beta (Settles & Craven 2008, eq. 1 with the density in place of the mean similarity): NumPy arrays
    or tensors, elementwise; beta = 0 leaves the utility, larger beta favours representative rows."""
    return utility * density ** beta


# ---- device form: every pool row against every reference row, nothing N x R stored ----------------------------------------
def information_density_device(rows, reference=None, want=("density",)):
    """Information density of a pool on the GPU (alink_information_density), Euclidean metric.

    rows       the pool, as in batch.ranked_batch_device: a CUDA float32 (N, D) tensor, or a tuple (left, right, li, ri) —
               row n is |left[li[n]] - right[ri[n]]|, formed on the fly, never materialised
    reference  None: the pool is its own reference (modAL's information_density); or a CUDA float32 (R, D) tensor, R >= 1:
               the rows to be near to — a sample of the pool, the gallery
    want       names among density (N,) float32: mean_j 1 / (1 + d(x_n, z_j)); mean_distance (N,) float32: mean_j d(x_n, z_j);
               central (1,) int32: the row with the least distance sum, ties to the lower index, a NaN never wins
    -> {name: CUDA tensor}.  Float32 distances in batch.hip's summation order, float64 sums (include/alink_hip.h pins the
    arithmetic).  Nothing is synchronised or read back except, in the pair form, the range check of li / ri."""
    import torch
    from . import _abi, net_host
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = [w for w in want if w not in DEVICE_OUTPUTS]
    if unknown or not want:
        raise ValueError("unknown density output(s) %s: choose among %s" % (unknown, list(DEVICE_OUTPUTS)))
    left, right, li, ri, N, D, dev = _pool_rows(rows, torch)
    if N < 1:
        raise ValueError("information_density_device: the pool is empty")
    if reference is not None:
        reference = _f32_matrix("reference", reference, torch, dev, D)
        if reference.shape[0] < 1:
            raise ValueError("reference: at least one row is needed (None: the pool is its own reference)")
    R = N if reference is None else reference.shape[0]
    lib = _abi.init(dev.index or 0)
    out = {w: torch.empty(1 if w == "central" else N, dtype=torch.int32 if w == "central" else torch.float32, device=dev) for w in want}
    sp = None
    if "central" in out:
        scratch, sp, _ = net_host.aligned_scratch(lib.alink_information_density_scratch_bytes(N), dev)
    _abi.check(lib.alink_information_density(_abi.ptr(left), _abi.ptr(right), _abi.ptr(li), _abi.ptr(ri), N, D, _abi.ptr(reference), R,
                                             *[_abi.ptr(out.get(w)) for w in DEVICE_OUTPUTS], sp, _abi.current_stream(dev)),
               "alink_information_density")
    return out
