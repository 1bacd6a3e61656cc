"""GPU: information density and the ranked batch's cold start on device (alink_information_density, density.hip) — bit equality
with the NumPy emulation of tests/test_density_host.py on inputs that admit no rounding in any order, the float64 values within
derived bounds on real-valued rows, the pair form against the row form, ties and NaNs, the cold ranked batch against the
emulation and the host, the Bagging entries, and what the library refuses."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

from test_density_host import COLD_SHAPES, EXACT_SHAPES, cold_case, emulate_cold, emulate_density, exact_case
from test_gpu_batch import _committee, _unit

pytestmark = pytest.mark.gpu
WANT = ("density", "mean_distance", "central")


def _dev(a):
    if isinstance(a, tuple):
        return tuple(_dev(x) for x in a)
    return None if a is None else torch.from_numpy(np.array(a)).cuda()           # (a copy: the shared cases are read-only)


def _run(rows, reference=None, want=WANT):
    from a_link_amd import density as Dn
    out = Dn.information_density_device(_dev(rows), _dev(reference), want=want)
    assert sorted(out) == sorted(want) and all(t.is_cuda for t in out.values())
    for w in want:
        assert out[w].dtype == (torch.int32 if w == "central" else torch.float32)
    got = {w: t.cpu().numpy() for w, t in out.items()}
    if "central" in got:
        assert got["central"].shape == (1,)
        got["central"] = int(got["central"][0])
    return got


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """got: _run's dict; want: emulate_density's tuple"""
    assert got["density"].shape == want[0].shape and got["mean_distance"].shape == want[1].shape
    assert np.array_equal(_bits(got["density"]), _bits(want[0]))
    assert np.array_equal(_bits(got["mean_distance"]), _bits(want[1]))
    assert got["central"] == want[2]


# (777, self, 40): N off the workgroup's 32 rows; (1031, self, 512): the register-resident form, 16-row tiles; (300, 2500, 7):
# D off 4 (scalar loads), R beyond one LDS tile (1,024 rows at D = 7), R off 4 and off 16; (65, self, 600): the any-D form,
# 13-row tiles — a group of sixteen never full; one row; one reference row; (40, self, 8192), features in {-1, 0, 1}: the D limit,
# one row per tile.  The kernel has no grid cap (one workgroup per 32 rows), so there is no sweep to go beyond.
@pytest.mark.parametrize("name", [s[0] for s in EXACT_SHAPES])
def test_bit_equal_to_the_emulation(gpu, name):
    X, Z, want = exact_case(name)
    _same(_run(X, Z), want)
    if name == "n_off_32":                                                   # every subset of the outputs, the same bits
        for sub in (("density",), ("mean_distance",), ("central",), ("central", "density")):
            got = _run(X, Z, want=sub)
            for w in sub:
                assert np.array_equal(got[w], want[WANT.index(w)])
        assert len(set(_bits(want[0]).tolist())) > 700                       # the densities tell the rows apart


def _pair_tables(rng, N, D, integer):
    nl, nr = 37, 11
    if integer:                                                              # in [-4, 4]: |l - r| in [0, 8]
        L, R = rng.randint(-4, 5, (nl, D)).astype(np.float32), rng.randint(-4, 5, (nr, D)).astype(np.float32)
    else:
        L, R = _unit(rng.randn(nl, D)), _unit(rng.randn(nr, D))
    return L, R, rng.randint(0, nl, N).astype(np.int32), rng.randint(0, nr, N).astype(np.int32)


@pytest.mark.parametrize("integer", [True, False])
@pytest.mark.parametrize("D", [512, 40, 7])
def test_pair_form_equals_row_form(gpu, D, integer):
    """row n = |L[li[n]] - R[ri[n]]| formed on the fly == the row form on the materialised rows, bit for bit, the pool as its
    own reference (its rows staged from the two tables) and with a reference table given.  D = 7 runs the scalar loads."""
    N, R = 1001, 77
    rng = np.random.RandomState(5 * D + integer)
    L, Rt, li, ri = _pair_tables(rng, N, D, integer)
    rows = np.abs(L[li] - Rt[ri])
    ref = rows[rng.randint(0, N, R)] + np.float32(1.0 if integer else 0.01)
    for Z in (None, ref):
        got_r, got_p = _run(rows, Z), _run((L, Rt, li, ri), Z)
        assert np.array_equal(_bits(got_p["density"]), _bits(got_r["density"]))
        assert np.array_equal(_bits(got_p["mean_distance"]), _bits(got_r["mean_distance"]))
        assert got_p["central"] == got_r["central"]
        if integer:
            _same(got_p, emulate_density(rows, Z))


def test_rows_off_the_vector_alignment(gpu):
    """a row table 4 bytes off a 16-byte boundary takes the scalar loads: same bits"""
    from a_link_amd import density as Dn
    X, _, want = exact_case("n_off_32")
    flat = torch.empty(X.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(*X.shape)
    view.copy_(torch.from_numpy(X))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    out = Dn.information_density_device(view, want=WANT)
    _same({"density": out["density"].cpu().numpy(), "mean_distance": out["mean_distance"].cpu().numpy(), "central": int(out["central"])}, want)


def test_equal_rows_ties_and_nans(gpu):
    # all rows equal: every distance 0, every similarity 1; the least sum is everybody's: the lowest index
    X = np.tile(np.arange(6, dtype=np.float32), (70, 1))
    got = _run(X)
    assert (got["density"] == 1.0).all() and (got["mean_distance"] == 0.0).all() and got["central"] == 0
    # two identical rows, in different workgroups, tie for the least sum: the lower index
    rng = np.random.RandomState(9)
    X = rng.randint(-8, 9, (600, 9)).astype(np.float32)
    c = emulate_density(X)[2]
    twin = (c + 300) % 600
    X[twin] = X[c]
    want = emulate_density(X)
    assert want[3][c] == want[3][twin] == want[3].min() and want[2] == min(c, twin)
    _same(_run(X), want)
    # a NaN sum never wins; nothing but NaN sums: -1
    Z = rng.randint(-8, 9, (50, 9)).astype(np.float32)
    want = emulate_density(X, Z)
    X[want[2], 3] = np.nan                                                   # the row that would have won
    want = emulate_density(X, Z)
    got = _run(X, Z)
    bad = np.isnan(X).any(axis=1)
    assert bad.sum() == 1 and got["central"] == want[2] and not bad[want[2]]
    assert np.isnan(got["density"][bad]).all() and np.isnan(got["mean_distance"][bad]).all()
    assert np.array_equal(_bits(got["density"][~bad]), _bits(want[0][~bad]))
    assert _run(X, want=("central",))["central"] == -1                       # its own reference: every row meets a NaN row
    assert _run(np.full((3, 4), np.nan, np.float32), Z[:, :4], want=("central",))["central"] == -1


@pytest.mark.parametrize("N,D", [(1003, 512), (1003, 40)])
def test_real_valued_rows_against_float64(gpu, N, D):
    """Rows |a - b| of unit vectors against float64 (direct differences), every element checked.  Let u = 2^-24 and
    e = ((D + 4) / 4 + 6) u, the relative error bound of the float32 d2 in its fixed summation order.
      d    = fl(sqrt(d2)): relative error e / 2 from d2 plus u for the rounding — e / 2 + u.
      mean distance: float64 sums of exact conversions add nothing that shows (R 2^-53); the quotient's cast to float32 adds u:
             |mean_distance - ref| <= (e / 2 + 2 u) ref.
      s    = fl(1 / fl(1 + d)): |ds| <= |dd| / (1 + d)^2 = (e / 2 + u) d / (1 + d)^2 <= (e / 2 + u) / 4; the rounded sum and
             the rounded division each add at most u s <= u; the final cast adds at most u (a density is at most 1):
             |density - ref| <= e / 8 + (13 / 4) u   (first order in u; the issue's 2^-22 = 4 u rounds this constant up).
      central: the device compares its float64 sums, each within b = e / 2 + u of the true one, relatively.  If it prefers row c
             to the true least row m then ref_c (1 - b) <= ref_m (1 + b), so ref_c - ref_m <= 2 b ref_c <= 2 (e / 2 + 2 u) ref_c.
    Seen on the MI355X: largest density error 1.6e-8 at both sizes (bounds 1.2e-6, 3.2e-7), largest relative mean-distance error
    5.1e-8 at D = 512 and 5.5e-8 at D = 40 (bounds 4.1e-6, 6.3e-7), and the central row is the float64 one."""
    rng = np.random.RandomState(7 + D)
    X = np.abs(_unit(rng.randn(N, D)) - _unit(rng.randn(N, D)))
    got = _run(X)
    u = 2.0 ** -24
    e = ((D + 4) / 4.0 + 6.0) * u
    dist = cdist(X.astype(np.float64), X.astype(np.float64))
    ref_density, ref_mean = (1.0 / (1.0 + dist)).mean(axis=1), dist.mean(axis=1)
    err_density = np.abs(got["density"].astype(np.float64) - ref_density)
    err_mean = np.abs(got["mean_distance"].astype(np.float64) - ref_mean) / ref_mean
    c = got["central"]
    print("D=%d: largest |density - float64| %.3e (bound %.3e), largest relative mean-distance error %.3e (bound %.3e), central %d "
          "(float64: %d), its float64 mean distance above the least by %.3e"
          % (D, err_density.max(), e / 8 + 3.25 * u, err_mean.max(), e / 2 + 2 * u, c, int(np.argmin(ref_mean)), ref_mean[c] - ref_mean.min()))
    assert got["density"].shape == (N,) and got["mean_distance"].shape == (N,) and 0 <= c < N
    assert (err_density <= e / 8 + 3.25 * u).all(), err_density.max()
    assert (err_mean <= e / 2 + 2 * u).all(), err_mean.max()
    assert ref_mean[c] - ref_mean.min() <= 2 * (e / 2 + 2 * u) * ref_mean[c]


def test_a_sampled_reference_is_the_rectangular_form(gpu):
    """a reference sample of the pool: the same numbers as the emulation against those rows, and self-pairs only where a row
    is in the sample"""
    X, _, _ = exact_case("n_off_32")
    sample = np.random.RandomState(3).choice(len(X), 100, replace=False)
    _same(_run(X, X[sample]), emulate_density(X, X[sample]))


@pytest.mark.parametrize("N,D,k", COLD_SHAPES)
def test_cold_ranked_batch(gpu, N, D, k):
    """picks [c] + rest: c the emulation's central row, rest the float32 emulation of the ranked-batch rule with that one row
    labelled over the other N - 1 rows, alpha_t = (N - 1 - t) / N; the same from the pair form; the host's picks."""
    from a_link_amd import batch as B
    L, R, li, ri, X, u = cold_case(N, D)
    want_idx, want_sc, _ = emulate_cold(X, u, k)
    assert want_idx[0] == emulate_density(X)[2] and len(want_idx) == min(k, N)
    idx, sc = B.ranked_batch_cold_device(_dev(X), _dev(u), k)
    assert idx.dtype == torch.int32 and sc.dtype == torch.float32 and idx.is_cuda and sc.is_cuda
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    assert idx.shape == (min(k, N),) and sc.shape == (min(k, N),)
    assert np.array_equal(idx, want_idx) and len(set(idx.tolist())) == len(idx) and idx.min() >= 0 and idx.max() < N
    assert np.isnan(sc[0]) and np.array_equal(_bits(sc[1:]), _bits(want_sc[1:]))
    idx_p, sc_p = B.ranked_batch_cold_device(_dev((L, R, li, ri)), _dev(u), k)
    assert np.array_equal(idx_p.cpu().numpy(), idx) and np.array_equal(_bits(sc_p.cpu().numpy()[1:]), _bits(sc[1:])) and bool(sc_p[0].isnan())

    class _Cold:
        X_training = None
    assert np.array_equal(B.ranked_batch(_Cold(), [L[li], R[ri]], u, k, "euclidean", None), idx)
    # a batch of one is the cold pick alone; a fixed alpha goes through
    idx1, sc1 = B.ranked_batch_cold_device(_dev(X), _dev(u), 1)
    assert idx1.cpu().tolist() == [int(want_idx[0])] and bool(sc1.isnan().all())
    idx0, _ = B.ranked_batch_cold_device(_dev(X), _dev(u), 5, alpha=0.0)     # alpha = 0: the central row, then the top utilities
    rest = np.argsort(-np.delete(u, want_idx[0]), kind="stable")[:4]
    assert np.array_equal(idx0.cpu().numpy()[1:], rest + (rest >= want_idx[0]))


def test_bagging_entries_and_errors(gpu):
    from a_link_amd import batch as B, density as Dn, uncertainty as U
    D, N, k = 64, 500, 24
    rng = np.random.RandomState(8)
    bag = _committee(D)
    L, R = torch.from_numpy(_unit(rng.randn(50, D))).cuda(), torch.from_numpy(_unit(rng.randn(9, D))).cuda()
    li = torch.from_numpy(rng.randint(0, 50, N).astype(np.int32)).cuda()
    ri = torch.from_numpy(rng.randint(0, 9, N).astype(np.int32)).cuda()
    rows = (L[li.long()] - R[ri.long()]).abs()
    reference = rows[::7].contiguous()
    for ref in (None, reference):
        got = bag.density_indexed(L, R, li, ri, reference=ref)
        assert got.shape == (N,) and got.dtype == torch.float32
        assert torch.equal(got, Dn.information_density_device((L, R, li, ri), ref)["density"])
        assert torch.equal(got, Dn.information_density_device(rows, ref)["density"])
    mean = bag.predict_indexed(L, R, li, ri)
    for kind in ("entropy", "uncertainty"):
        got_idx, got_sc = bag.ranked_batch_cold_indexed(L, R, li, ri, k, kind=kind)
        util = U.score_device(mean, kind)
        for pool in ((L, R, li, ri), rows):
            want_idx, want_sc = B.ranked_batch_cold_device(pool, util, k)
            assert got_idx.shape == (k,) and torch.equal(got_idx, want_idx) and torch.equal(got_sc[1:], want_sc[1:]) and bool(got_sc[0].isnan())
    got_idx, _ = bag.ranked_batch_cold_indexed(L, R, li, ri, k, kind="vote_entropy", alpha=0.5)
    want_idx, _ = B.ranked_batch_cold_device((L, R, li, ri), bag.disagreement_indexed(L, R, li, ri, kind="vote_entropy"), k, alpha=0.5)
    assert torch.equal(got_idx, want_idx)
    # density weighting on the device: plain elementwise work on the two vectors
    util = U.score_device(mean, "entropy")
    dens = bag.density_indexed(L, R, li, ri)
    assert torch.equal(Dn.density_weighted(util, dens, beta=2.0), util * dens ** 2.0)
    # refused by the Python entries
    with pytest.raises(ValueError, match="margin"):
        bag.ranked_batch_cold_indexed(L, R, li, ri, k, kind="margin")
    with pytest.raises(ValueError, match="one feature space"):
        bag.ranked_batch_cold_indexed([L, L], [R, R], li, ri, k)
    with pytest.raises(ValueError, match="one feature space"):
        bag.density_indexed([L, L], [R, R], li, ri)
    with pytest.raises(ValueError, match="CUDA"):
        Dn.information_density_device((L.cpu(), R, li, ri))
    with pytest.raises(ValueError, match="CUDA"):
        Dn.information_density_device((L, R, li, ri), reference.cpu())
    with pytest.raises(ValueError, match="float32"):
        Dn.information_density_device((L.double(), R, li, ri))
    with pytest.raises(ValueError, match="float32"):
        Dn.information_density_device(rows, reference.double())
    with pytest.raises(ValueError, match="int32"):
        Dn.information_density_device((L, R, li.long(), ri))
    with pytest.raises(ValueError, match="D = 63"):
        Dn.information_density_device((L, R, li, ri), reference[:, :63])
    with pytest.raises(ValueError, match="D = 32"):
        Dn.information_density_device((L, R[:, :32], li, ri))
    with pytest.raises(ValueError, match="outside its table"):
        Dn.information_density_device((L, R, li, ri + 1))
    with pytest.raises(ValueError, match="at least one row"):
        Dn.information_density_device(rows, reference[:0])
    with pytest.raises(ValueError, match="unknown density output"):
        Dn.information_density_device(rows, want=("median",))
    with pytest.raises(ValueError, match="utility"):
        B.ranked_batch_cold_device((L, R, li, ri), util[:-1], k)
    with pytest.raises(ValueError, match="alpha"):
        B.ranked_batch_cold_device((L, R, li, ri), util, k, alpha=1.5)
    with pytest.raises(ValueError, match="n_instances"):
        B.ranked_batch_cold_device((L, R, li, ri), util, 0)
    with pytest.raises(ValueError, match="at least one labelled row"):       # the warm form still refuses M = 0
        B.ranked_batch_device((L, R, li, ri), util, rows[:0], k)


def test_limits_the_library_refuses(gpu):
    lib = gpu.load()
    x = torch.zeros((8, 4), device="cuda")
    dens = torch.full((8,), -7.0, device="cuda")
    mean = torch.full((8,), -7.0, device="cuda")
    central = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    scratch = torch.empty(lib.alink_information_density_scratch_bytes(8) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(N=8, D=4, ref=x, R=8, outputs=(dens, mean, central), scratch_ptr=sp):
        return lib.alink_information_density(gpu.ptr(x), None, None, None, N, D, gpu.ptr(ref), R, *[gpu.ptr(o) for o in outputs],
                                             C.c_void_p(scratch_ptr), st)
    for kw, text in ((dict(N=0), "N=0"), (dict(N=2 ** 31), "N=2147483648"), (dict(R=0), "R=0"), (dict(R=2 ** 31), "R=2147483648"),
                     (dict(D=0), "D=0"), (dict(D=8193), "D=8193"), (dict(outputs=(None, None, None)), "no output"),
                     (dict(ref=None, R=5), "its own reference"), (dict(scratch_ptr=sp + 4), "aligned"), (dict(scratch_ptr=0), "scratch")):
        assert call(**kw) == -1, kw                                           # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(R=0), "alink_information_density")
    torch.cuda.synchronize()
    assert bool((dens == -7).all()) and bool((mean == -7).all()) and int(central) == -7      # a refused call launches nothing
    assert call(outputs=(dens, None, None), scratch_ptr=0) == 0               # scratch is the central row's alone
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((dens == 1).all()) and bool((mean == 0).all()) and int(central) == 0          # eight identical rows
