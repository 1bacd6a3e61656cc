"""GPU: BAIT on the device (bait.hip) through the C ABI — the factor rows against the float64 host under a
tolerance measured in the same test, the score pass bit for bit on integer data, the selection loop
against the float64 host rule on the device's own factor rows (forced replay, near-ties excused inside a measured band), its
state and bookkeeping, and the end-to-end routes."""
import functools

import numpy as np
import pytest
import torch

from oracle import siamese_head as O
from test_egl_host import make_case

pytestmark = pytest.mark.gpu

SHAPE = (64, 128, 64, 2)                           # D, h1, h2, od of the selection tests
N_SEL, N_LAB = 2000, 20
SEED = 2
TILE = 128


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def make_head(shape, ws):
    from a_link_amd.head import DenseHead
    D, h1, h2, od = shape
    head = DenseHead(D, h1=h1, h2=h2, lr=0.1, seed=1, out_dim=od)
    head.set_weights(ws)
    return head


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---- 1. factor -------------------------------------------------------------------------------------------------------------
def restate32(ws, L, R):
    """the head's forward, egl's embedding and the factor rule in float32 NumPy"""
    from a_link_amd import bait
    f = np.float32
    p, (d, z1, a1, z2, a2) = O.forward([np.asarray(w, f) for w in ws], L.astype(f), R.astype(f), dtype=f, cache=True)
    p, a2 = np.asarray(p, f), np.asarray(a2, f)
    hit = np.zeros_like(p)
    if p.shape[1] == 2:
        hit[np.arange(len(p)), (p[:, 1] > p[:, 0]).astype(int)] = 1
    else:
        hit[:, 0] = p[:, 0] > 0.5
    emb = ((p - hit)[:, :, None] * a2[:, None, :]).reshape(len(p), -1).astype(f)
    return bait.factor_from_outputs(p, emb, dtype=f)


def row_error(got, want):
    """largest error of a row relative to the row's largest entry (rows of zeros: absolute)"""
    scale = np.maximum(np.abs(want).max(axis=1), 1e-30)
    return float((np.abs(got.astype(np.float64) - want).max(axis=1) / scale).max())


@pytest.mark.parametrize("shape", [(64, 128, 64, 2), (40, 128, 32, 1)], ids=["softmax", "sigmoid"])
def test_factor_rows_against_the_float64_host(gpu, shape):
    from a_link_amd import bait
    ws, L, R = make_case(*shape, n=300, seed=1)
    want = bait.fisher_factor(ws, [L, R])
    head = make_head(shape, ws)
    out = head.expected_gradient_length_device(dev(L), dev(R), want=("probs", "emb"))
    f = bait.fisher_factor_device(out["probs"], out["emb"]).cpu().numpy()
    assert f.shape == want.shape and f.dtype == np.float32
    live = np.abs(want).max(axis=1) > 0
    assert live.sum() > 200
    err32 = row_error(restate32(ws, L, R)[live], want[live])
    err = row_error(f[live], want[live])
    print("factor rows, %s: device %.2e, float32 NumPy %.2e of the row's largest entry" % (shape, err, err32))
    assert err <= 4 * err32
    assert (f[~live] == 0).all()
    # the device's rule on the device's own outputs, restated in float32: one product per element, the same bits
    again = bait.factor_from_outputs(out["probs"].cpu().numpy(), out["emb"].cpu().numpy(), dtype=np.float32)
    assert np.array_equal(bits(f), bits(again))


def test_saturated_rows_are_exactly_zero(gpu):
    from a_link_amd import bait
    for shape in ((64, 128, 64, 2), (40, 128, 32, 1)):
        ws, L, R = make_case(*shape, n=70, seed=1)
        ws = [w.copy() for w in ws]
        ws[5] = ws[5] + (np.array([60.0, -60.0], np.float32) if shape[3] == 2 else np.float32(60.0))
        out = make_head(shape, ws).expected_gradient_length_device(dev(L), dev(R), want=("probs", "emb"))
        f = bait.fisher_factor_device(out["probs"], out["emb"]).cpu().numpy()
        p = out["probs"].cpu().numpy()
        sat = ((p < np.float32(1e-7)) | (p > np.float32(1) - np.float32(1e-7))).any(axis=1)
        assert sat.sum() >= 60                                                  # (a row scaled by 64 may stay inside)
        assert f.shape == (70, shape[2]) and not f[sat].any() and f[~sat].any() == (~sat).any()


# ---- 3. scores -------------------------------------------------------------------------------------------------------------
def integer_case(N, F, m, seed):
    """integer f (|f| <= 3), integer A (|A| <= 2), B = G^T G for a 4-row G of -1 / 0 / 1 that touches the first 4 columns only:
    every quadratic form and every partial sum of one is an integer below 2^24 (q_A <= 18 F^2, q_B <= 4 (3 x 4)^2), and a row
    whose first 4 entries are 0 in every block has q_B = 0 — the rows the backward form does not skip"""
    rng = np.random.RandomState(seed)
    f = rng.randint(-3, 4, (N, m * F)).astype(np.float32)
    quiet = rng.rand(N) < 0.5
    for j in range(m):
        f[quiet, j * F:j * F + 4] = 0
    A = rng.randint(-2, 3, (m, F, F)).astype(np.float64)                       # NOT symmetric: a transposed read would show
    G = np.zeros((m, 4, F))
    G[:, :, :4] = rng.randint(-1, 2, (m, 4, 4))
    B = np.einsum("mri,mrj->mij", G, G)
    return f, A, B


def host_best(scores, free):
    from a_link_amd import bait
    return bait.first_argmax(scores.astype(np.float64), free)


@pytest.mark.parametrize("F,m", [(F, m) for F in (8, 32, 64, 128) for m in (1, 3)])
def test_scores_and_best_index_on_integer_data_bit_for_bit(gpu, F, m):
    from a_link_amd import bait
    for N in (TILE - 1, TILE, TILE + 1, 3 * TILE + 5, 1):
        f, A, B = integer_case(N, F, m, seed=N + F + m)
        AB = dev(bait.pack_ab(A, B))
        rng = np.random.RandomState(N)
        free = (rng.rand(N) < 0.7).astype(np.uint8)                            # a mask with picked rows
        for sign in (1, -1):
            want = bait.bait_scores(f, A, B, sign=sign, blocks=m, dtype=np.float32)
            assert want.dtype == np.float32
            if sign < 0 and N > 1:
                assert np.isnan(want).any() and not np.isnan(want).all()       # the q_B >= 1 skip is exercised, and so is its absence
            for mask in (free, np.ones(N, np.uint8), np.zeros(N, np.uint8)):
                scores, partial = bait.bait_scores_device(dev(f), AB, dev(mask), sign=sign, blocks=m)
                got = scores.cpu().numpy()
                assert np.array_equal(np.isnan(got), np.isnan(want)), (N, F, m, sign)
                ok = ~np.isnan(want)
                assert np.array_equal(bits(got[ok]), bits(want[ok])), (N, F, m, sign)
                assert partial.shape == ((N + TILE - 1) // TILE, 2)
                best = bait.best_of_partials(partial)
                n = host_best(want, mask.astype(bool))
                assert best[1] == n, (N, F, m, sign, best, n)
                if n >= 0:
                    assert np.float32(best[0]) == want[n]
    # without the scores output the partial maxima are the same: a shape with free rows in every tile
    N = 3 * TILE + 5
    f, A, B = integer_case(N, F, m, seed=N + F + m)
    AB, mask = dev(bait.pack_ab(A, B)), dev((np.random.RandomState(N).rand(N) < 0.7).astype(np.uint8))
    for sign in (1, -1):
        _, p1 = bait.bait_scores_device(dev(f), AB, mask, sign=sign, blocks=m)
        _, p2 = bait.bait_scores_device(dev(f), AB, mask, sign=sign, blocks=m, want_scores=False)
        assert torch.equal(p2, p1) and (p1[:, 1] != 0x7fffffff).all()


def test_equal_scores_give_the_lowest_index(gpu):
    from a_link_amd import bait
    F, N = 32, 3 * TILE + 5
    f, A, B = integer_case(1, F, 1, seed=5)
    f = np.repeat(f, N, axis=0)
    AB = dev(bait.pack_ab(A, B))
    free = np.ones(N, np.uint8)
    assert bait.best_of_partials(bait.bait_scores_device(dev(f), AB, dev(free))[1])[1] == 0
    free[:TILE + 3] = 0
    assert bait.best_of_partials(bait.bait_scores_device(dev(f), AB, dev(free))[1])[1] == TILE + 3


@pytest.mark.parametrize("F,m", [(8, 1), (64, 1), (128, 3), (40, 2)])
def test_a_rows_score_does_not_depend_on_its_place(gpu, F, m):
    """real-valued data: the same bits alone, in the middle of a pool, and in a permuted pool"""
    from a_link_amd import bait
    rng = np.random.RandomState(F)
    N = 2 * TILE + 37
    f = rng.randn(N, m * F).astype(np.float32)
    G = rng.randn(m, F, F) / F                                                  # q_B on both sides of 1
    B = np.einsum("mri,mrj->mij", G, G)
    A = B @ B
    AB = dev(bait.pack_ab(A, B))
    free = dev(np.ones(N, np.uint8))
    for sign in (1, -1):
        pool = bait.bait_scores_device(dev(f), AB, free, sign=sign, blocks=m)[0].cpu().numpy()
        want = bait.bait_scores(f, A, B, sign=sign, blocks=m)
        if sign > 0:                                        # (backward, q_B - 1 cancels next to 1: only the bits are compared there)
            assert np.abs(pool - want).max() <= 1e-4 * np.abs(want).max()
        else:
            assert 0 < np.isnan(pool).sum() < N
        for n in (0, TILE + 9, N - 1):
            alone = bait.bait_scores_device(dev(f[n:n + 1]), AB, free[:1], sign=sign, blocks=m)[0].cpu().numpy()
            assert np.array_equal(bits(alone), bits(pool[n:n + 1]))
        perm = rng.permutation(N)
        mixed = bait.bait_scores_device(dev(f[perm]), AB, free, sign=sign, blocks=m)[0].cpu().numpy()
        assert np.array_equal(bits(mixed), bits(pool[perm]))


# ---- 4. select -------------------------------------------------------------------------------------------------------------
def top_two(s):
    """(best index, relative gap between the two largest) of a score vector with -inf for what may not be taken"""
    n1 = int(np.argmax(s))
    rest = s.copy()
    rest[n1] = -np.inf
    s2 = rest.max()
    gap = (s[n1] - s2) / abs(s[n1]) if np.isfinite(s2) and s[n1] != 0 else np.inf
    return n1, gap


def replay(f64, phi, M0, free, forward, final, k, m, band):
    """the float64 host rule forced along the device's picks: a device pick may differ from the host's only when the host scores
    the two within `band` of each other (relative to the best).  -> (steps excused, smallest top-two gap met, steps, B)"""
    from a_link_amd import bait
    B = np.stack([np.linalg.inv(M0[j]) for j in range(m)])
    free = free.copy()
    excused, mingap, steps = 0, np.inf, 0
    for d in forward:
        A = np.stack([B[j] @ phi[j] @ B[j] for j in range(m)])
        s = bait.bait_scores(f64, A, B, 1, m)
        s = np.where(free & ~np.isnan(s), s, -np.inf)
        n1, gap = top_two(s)
        mingap, steps = min(mingap, gap), steps + 1
        assert free[d], "the device picked row %d, which is not free" % d
        if d != n1:
            rel = (s[n1] - s[d]) / abs(s[n1])
            assert rel < band, "forward step %d: device %d, host %d, apart by %.3e of the best (band %.3e)" % (steps - 1, d, n1, rel, band)
            excused += 1
        free[d] = False
        B = bait.woodbury(B, f64[d], 1, m)
    kept, removed = list(forward), set(forward) - set(final)
    while len(kept) > k:
        A = np.stack([B[j] @ phi[j] @ B[j] for j in range(m)])
        s = bait.bait_scores(f64[kept], A, B, -1, m)
        s = np.where(np.isnan(s), -np.inf, s)
        r1, gap = top_two(s)
        mingap, steps = min(mingap, gap), steps + 1
        r = max((i for i in range(len(kept)) if kept[i] in removed), key=lambda i: (s[i], -i))
        if r != r1:
            rel = (s[r1] - s[r]) / abs(s[r1])
            assert rel < band, "prune step: device removed %d, host %d, apart by %.3e (band %.3e)" % (kept[r], kept[r1], rel, band)
            excused += 1
        B = bait.woodbury(B, f64[kept[r]], -1, m)
        removed.discard(kept[r])
        del kept[r]
    assert kept == list(final), "the kept rows are not in the order they were picked"
    return excused, mingap, steps, B


@functools.lru_cache(maxsize=None)
def selection_case():
    """computed once: the head, N_SEL pairs, the device's factor rows and everything the host derives from them"""
    from a_link_amd import bait
    ws, L, R = make_case(*SHAPE, n=N_SEL, seed=SEED)
    head = make_head(SHAPE, ws)
    out = head.expected_gradient_length_device(dev(L), dev(R), want=("probs", "emb"))
    f = bait.fisher_factor_device(out["probs"], out["emb"])
    f64 = f.cpu().numpy().astype(np.float64)
    lab = np.random.RandomState(SEED).choice(N_SEL, N_LAB, replace=False)
    free = np.ones(N_SEL, bool)
    free[lab] = False
    phi = bait.fisher_matrix(f64, scale=1.0 / N_SEL)
    M0 = np.eye(SHAPE[2])[None] + bait.fisher_matrix(f64, rows=lab)
    B0 = np.linalg.inv(M0)
    B0 = 0.5 * (B0 + B0.transpose(0, 2, 1))
    s64 = bait.bait_scores(f64, B0 @ phi @ B0, B0)
    s32 = bait.bait_scores(f64.astype(np.float32), B0 @ phi @ B0, B0, dtype=np.float32)
    err = float(np.abs(s32 - s64).max() / np.abs(s64).max())
    for a in (f64, lab, free, phi, M0, B0):
        a.setflags(write=False)
    return dict(head=head, ws=ws, L=L, R=R, f=f, f64=f64, lab=lab, free=free, phi=phi, M0=M0, B0=B0, err=err)


def run_select(c, k_forward, k_keep, B=None, free=None):
    from a_link_amd import bait
    B = dev(c["B0"]) if B is None else B
    free = dev(c["free"].astype(np.uint8)) if free is None else free
    idx, score = bait.bait_select_device(c["f"], dev(c["phi"]), B, free, k_forward, k_keep)
    return idx, score, B, free


@pytest.mark.parametrize("k", [8, 32])
def test_select_against_the_float64_host_on_the_devices_rows(gpu, k):
    from a_link_amd import bait
    c = selection_case()
    band = 4 * c["err"]
    fwd = run_select(c, 2 * k, 2 * k)[0].cpu().numpy()
    idx, score, B, free = run_select(c, 2 * k, k)
    got = idx.cpu().numpy()
    assert len(set(got)) == k and set(got) <= set(fwd) and not set(got) & set(c["lab"]) and (got >= 0).all()
    excused, mingap, steps, Bhost = replay(c["f64"], c["phi"], c["M0"], c["free"], list(fwd), list(got), k, 1, band)
    print("k = %d: %d of %d steps excused; smallest top-two gap %.2e, float32 score error %.2e, band %.2e" % (k, excused, steps, mingap, c["err"], band))
    assert excused <= 0.05 * steps
    if excused == 0:
        want, Bwant = bait.bait_select(c["f64"], c["phi"], c["M0"], k, free=c["free"])
        assert np.array_equal(got, want)
        assert np.abs(Bwant - Bhost).max() <= 1e-12 * np.abs(Bwant).max()
    Bdev = B.cpu().numpy()
    rel = np.abs(Bdev - Bhost).max() / np.abs(Bhost).max()
    print("k = %d: B out against the host's, relative %.2e" % (k, rel))
    assert rel <= 1e-9
    # the free bytes: cleared on the labelled rows and on the rows returned, nowhere else
    want_free = c["free"].copy()
    want_free[got] = False
    assert np.array_equal(free.cpu().numpy().astype(bool), want_free)
    # the scores are the forward scores the rows were picked at
    pos = {n: t for t, n in enumerate(fwd)}
    fs = run_select(c, 2 * k, 2 * k)[1].cpu().numpy()
    assert np.array_equal(bits(score), bits(fs[[pos[n] for n in got]]))


def test_chained_calls_equal_one_call_and_runs_repeat(gpu):
    c = selection_case()
    k1, k2 = 11, 21
    one = run_select(c, k1 + k2, k1 + k2)
    a = run_select(c, k1, k1)
    b = run_select(c, k2, k2, B=a[2], free=a[3])
    assert torch.equal(torch.cat([a[0], b[0]]), one[0])
    assert np.array_equal(bits(torch.cat([a[1], b[1]])), bits(one[1]))
    assert np.array_equal(bits(b[2]), bits(one[2])) and torch.equal(b[3], one[3])
    assert not set(a[0].tolist()) & set(b[0].tolist())                              # picked rows are never returned again
    for k_forward, k_keep in ((k1 + k2, k1 + k2), (32, 16)):
        x, y = run_select(c, k_forward, k_keep), run_select(c, k_forward, k_keep)
        assert torch.equal(x[0], y[0]) and np.array_equal(bits(x[1]), bits(y[1])) and np.array_equal(bits(x[2]), bits(y[2]))


def test_fewer_free_rows_than_picks_and_the_c_refusals(gpu):
    import ctypes as C
    from a_link_amd import bait
    _abi = gpu
    c = selection_case()
    free = np.zeros(N_SEL, np.uint8)
    free[[7, 300, 1999]] = 1
    idx, score, B, fr = run_select(c, 5, 5, free=dev(free))
    assert sorted(idx.tolist()[:3]) == [7, 300, 1999] and idx.tolist()[3:] == [-1, -1] and not fr.any()
    assert np.isnan(score.cpu().numpy()[3:]).all()
    # ... and with a prune: 3 forward picks are found, so ONE row is removed on the way to k_keep = 2, not k_forward - k_keep = 3
    idx, score, B, fr = run_select(c, 5, 2, free=dev(free))
    want, Bwant = bait.bait_select(c["f64"], c["phi"], c["M0"], 2, over=2, free=free.astype(bool))
    assert len(want) == 2 and np.array_equal(idx.cpu().numpy(), want) and not np.isnan(score.cpu().numpy()).any()
    assert np.abs(B.cpu().numpy() - Bwant).max() <= 1e-9 * np.abs(Bwant).max()
    left = free.copy()
    left[want] = 0
    assert np.array_equal(fr.cpu().numpy(), left)                                  # the row removed is free again
    idx, _, _, fr = run_select(c, 5, 3, free=dev(free))                           # as many kept as asked for: nothing is removed
    assert sorted(idx.tolist()) == [7, 300, 1999] and not fr.any()
    idx, _, _, _ = run_select(c, 5, 4, free=dev(free))
    assert sorted(idx.tolist()[:3]) == [7, 300, 1999] and idx.tolist()[3] == -1
    lib = _abi.init(0)
    f, phi, B, fr = c["f"], dev(c["phi"]), dev(c["B0"]), dev(free)
    out_i, out_s = torch.full((4,), 77, dtype=torch.int32, device="cuda"), torch.zeros(4, device="cuda")
    scratch = torch.empty(lib.alink_bait_select_scratch_bytes(N_SEL, 64, 1, 8) + 256, dtype=torch.uint8, device="cuda")
    sp = scratch.data_ptr() + (-scratch.data_ptr()) % 256
    p, st = _abi.ptr, _abi.current_stream(0)
    bad = [
        lambda: lib.alink_bait_select(None, N_SEL, 64, 1, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), 0, 64, 1, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 60, 1, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 136, 1, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 64, 9, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 128, 5, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 64, 1, p(phi), p(B), p(fr), 4, 0, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 64, 1, p(phi), p(B), p(fr), 3, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 64, 1, p(phi), p(B), p(fr), N_SEL + 1, 4, p(out_i), p(out_s), sp, st),
        lambda: lib.alink_bait_select(p(f), N_SEL, 64, 1, p(phi), p(B), p(fr), 4, 4, p(out_i), p(out_s), C.c_void_p(sp + 8), st),
        lambda: lib.alink_bait_scores(p(f), N_SEL, 64, 1, p(phi), p(fr), 0, None, p(out_i), st),
        lambda: lib.alink_bait_scores(p(f), N_SEL, 64, 1, None, p(fr), 1, None, p(out_i), st),
        lambda: lib.alink_fisher_factor(p(f), p(f), 10, 3, 64, p(out_s), st),
    ]
    for i, call in enumerate(bad):
        assert call() == -1, i
    torch.cuda.synchronize()
    assert out_i.tolist() == [77] * 4 and np.array_equal(B.cpu().numpy(), c["B0"])   # nothing was launched
    assert lib.alink_bait_select_scratch_bytes(N_SEL, 60, 1, 8) == 0
    for call in (lambda: bait.bait_select_device(c["f"], phi, B, fr, 4, 5), lambda: bait.bait_select_device(c["f"], phi, B.float(), fr, 4, 4),
                 lambda: bait.bait_select_device(c["f"], phi, B, fr.bool(), 4, 4), lambda: bait.bait_select_device(c["f"][:, :60], phi, B, fr, 4, 4),
                 lambda: bait.bait_factors_device(c["f"], np.arange(N_SEL), 4), lambda: bait.bait_factors_device(c["f"], None, 0)):
        with pytest.raises(ValueError):
            call()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def check_route(f, lab, k, m, got):
    """a route's picks against the host rule on the device's own factor rows, under the excusal rule of the selection test"""
    from a_link_amd import bait
    N, F = f.shape[0], f.shape[1] // m
    f64 = f.cpu().numpy().astype(np.float64)
    free = np.ones(N, bool)
    free[lab] = False
    phi = bait.fisher_matrix(f64, scale=1.0 / N, blocks=m)
    M0 = np.eye(F)[None] + bait.fisher_matrix(f64, rows=lab, blocks=m)
    B0 = np.linalg.inv(M0)
    B0 = 0.5 * (B0 + B0.transpose(0, 2, 1))
    A0 = B0 @ phi @ B0
    err = float(np.abs(bait.bait_scores(f64.astype(np.float32), A0, B0, blocks=m, dtype=np.float32) - bait.bait_scores(f64, A0, B0, blocks=m)).max()
                / np.abs(bait.bait_scores(f64, A0, B0, blocks=m)).max())
    kf = min(2 * k, int(free.sum()))
    # the route's forward picks: the same call without the prune
    fwd = bait.bait_select_device(f, dev(phi), dev(B0), dev(free.astype(np.uint8)), kf, kf, blocks=m)[0].cpu().numpy()
    excused, mingap, steps, _ = replay(f64, phi, M0, free, list(fwd), list(got), k, m, 4 * err)
    print("route with %d block(s): %d of %d steps excused; smallest gap %.2e, float32 score error %.2e" % (m, excused, steps, mingap, err))
    assert excused <= 0.05 * steps
    if excused == 0:
        assert np.array_equal(got, bait.bait_select(f64, phi, M0, k, blocks=m, free=free)[0])


def test_bait_device_and_the_sampler(gpu):
    from a_link_amd import bait
    c = selection_case()
    head, k = c["head"], 10
    dL, dR = dev(c["L"]), dev(c["R"])
    idx, score = head.bait_device(dL, dR, labelled=c["lab"], n_instances=k)
    got = idx.cpu().numpy()
    assert idx.dtype == torch.int32 and len(set(got)) == k and not set(got) & set(c["lab"])
    check_route(c["f"], c["lab"], k, 1, got)
    # indexed pairs: the same pairs gathered by index give the same picks
    rng = np.random.RandomState(4)
    perm_l, perm_r = rng.permutation(N_SEL), rng.permutation(N_SEL)
    li, ri = dev(np.argsort(perm_l).astype(np.int32)), dev(np.argsort(perm_r).astype(np.int32))
    idx2, _ = bait.bait_device(head, dev(c["L"][perm_l]), dev(c["R"][perm_r]), li, ri, labelled=c["lab"], n_instances=k)
    assert torch.equal(idx2, idx)
    # the modAL-shaped sampler on CUDA tensors: nothing labelled
    q, inst = bait.bait_sampling(head, [dL, dR], n_instances=k)
    assert q.dtype == np.int64 and len(set(q)) == k
    check_route(c["f"], np.zeros(0, np.int64), k, 1, q)
    assert torch.equal(inst[0], dL[torch.from_numpy(q).cuda()]) and torch.equal(inst[1], inst[0])

    class Host(object):
        def get_weights(self):
            return c["ws"]
    with pytest.raises(TypeError, match="DenseHead"):
        bait.bait_sampling(Host(), [dL, dR])


def test_committee_rows_are_the_members_factors_side_by_side(gpu):
    from a_link_amd import bait, committee, siamese
    D, n_pairs, k = 64, 600, 12
    rng = np.random.RandomState(9)
    nets = []
    for m in range(2):
        net = siamese.SiameseNetwork((D,), "e%d" % m, 0.1, seed=60 + m)
        ws = net.siamese_net.get_weights()
        ws[4] = ws[4] * np.float32(40.0)                                            # probabilities spread over (0, 1)
        net.siamese_net.set_weights(ws)
        nets.append(net)
    bag = committee.Bagging(nets, [])
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    L, R = dev(unit(rng.randn(40, D))), dev(unit(rng.randn(9, D)))
    li, ri = dev(rng.randint(0, 40, n_pairs).astype(np.int32)), dev(rng.randint(0, 9, n_pairs).astype(np.int32))
    labelled = rng.permutation(n_pairs)[:30]
    idx, score = bag.bait_indexed(L, R, li, ri, labelled, k)
    got = idx.cpu().numpy()
    assert len(set(got)) == k and not set(got) & set(labelled) and (got >= 0).all()
    fs = []
    for net in nets:
        out = net.siamese_net.expected_gradient_length_device(L, R, li, ri, want=("probs", "emb"))
        fs.append(bait.fisher_factor_device(out["probs"], out["emb"]))
    check_route(torch.cat(fs, dim=1), labelled, k, 2, got)

    with pytest.raises(ValueError, match="512"):
        committee.Bagging([siamese.SiameseNetwork((D,), "w%d" % i, 0.1, seed=i) for i in range(9)], []).bait_indexed(L, R, li, ri, labelled, k)

    class Host(object):
        siamese_net = None
    with pytest.raises(TypeError, match="DenseHead"):
        committee.Bagging([Host()], []).bait_indexed(L, R, li, ri, labelled, k)
