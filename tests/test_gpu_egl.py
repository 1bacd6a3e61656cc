"""GPU: expected gradient length and gradient embedding on device (alink_head_egl, egl.hip) — parity with the float64 oracle
loop under a tolerance measured in the same test, exact zeros on saturated rows, bit equalities (the forward's probabilities,
indexed against materialised rows, a pair alone against the pair in a pool, one output against all three), weights that move,
the committee mean and the ranked batch on it, and every refusal."""
import functools

import numpy as np
import pytest
import torch

from oracle import siamese_head as O
from test_egl_host import N, SCALED, SHAPES, make_case, oracle_loop

pytestmark = pytest.mark.gpu

GPU_SHAPES = SHAPES + [(520, 256, 64, 2)]          # the last crosses the 512-deep K chunk
IDS = ["D%d_h%d_%d_od%d" % s for s in GPU_SHAPES]
FLOOR_ULPS = 16                                    # MFMA's k-ordered chain and NumPy's BLAS order the sums differently
MASK_MARGIN = 2e-5                                 # |z1| or |z2| below it: a relu mask may legitimately flip in float32


def closed_form(ws, L, R, dtype):
    """the closed form of egl.py evaluated in `dtype` NumPy on the oracle's forward cache -> (egl (N,), emb (N, od * h2))"""
    p, (d, z1, a1, z2, a2) = O.forward(ws, L, R, dtype=dtype, cache=True)
    W2, W3 = np.asarray(ws[2], dtype), np.asarray(ws[4], dtype)
    od = p.shape[1]
    wd = W3[:, 0] - W3[:, 1] if od == 2 else W3[:, 0]
    u = wd[None, :] * (z2 > 0)
    v = (u @ W2.T) * (z1 > 0)
    sq = lambda a: (a * a).sum(axis=1, dtype=dtype)
    g2 = dtype(od) * (sq(a2) + dtype(1)) + sq(u) * (sq(a1) + dtype(1)) + sq(v) * (sq(d) + dtype(1))
    pq = p[:, 0] * p[:, 1] if od == 2 else p[:, 0] * (dtype(1) - p[:, 0])
    eps = dtype(1e-7)
    inside = ((p >= eps) & (p <= dtype(1) - eps)).all(axis=1)
    hit = np.zeros_like(p)
    if od == 2:
        hit[np.arange(len(p)), (p[:, 1] > p[:, 0]).astype(int)] = 1
    else:
        hit[:, 0] = p[:, 0] > dtype(0.5)
    dz = np.where(inside[:, None], p - hit, dtype(0))
    emb = (dz[:, :, None] * a2[:, None, :]).reshape(len(p), -1)
    return np.where(inside, dtype(2) * pq * np.sqrt(g2), dtype(0)).astype(dtype), emb.astype(dtype)


@functools.lru_cache(maxsize=None)
def reference(shape):
    """computed once per shape and left unchanged: inputs, the float64 oracle loop, the float32 NumPy closed form, row classes"""
    ws, L, R = make_case(*shape)
    egl64, emb64, p64, margin = oracle_loop(ws, L, R)
    egl32, emb32 = closed_form(ws, L, R, np.float32)
    pmax = p64.max(axis=1) if p64.shape[1] == 2 else np.maximum(p64[:, 0], 1 - p64[:, 0])
    saturated = 1 - pmax < 1e-9
    between = (1 - pmax >= 1e-9) & (1 - pmax < 1e-4)
    near_mask = margin < MASK_MARGIN
    for a in (L, R, egl64, emb64, p64, egl32, emb32, saturated, between, near_mask):
        a.setflags(write=False)
    return dict(ws=ws, L=L, R=R, egl64=egl64, emb64=emb64, p64=p64, egl32=egl32, emb32=emb32, saturated=saturated, between=between,
                near_mask=near_mask)


def make_head(shape, ws=None):
    from a_link_amd.head import DenseHead
    D, h1, h2, od = shape
    head = DenseHead(D, h1=h1, h2=h2, lr=0.1, seed=1, out_dim=od)
    if ws is not None:
        head.set_weights(ws)
    return head


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()              # a copy: the references are read-only


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


ALL = ("egl", "probs", "emb")


@functools.lru_cache(maxsize=None)
def device_run(shape):
    """all three outputs of the whole 70-pair case, once per shape -> (head, {name: tensor})"""
    ref = reference(shape)
    head = make_head(shape, ref["ws"])
    return head, head.expected_gradient_length_device(dev(ref["L"]), dev(ref["R"]), want=ALL)


def compared_rows(ref, P):
    """(rows of the first P that the parity checks compare, saturated rows that must be exactly zero).  Left out: rows with a
    |z1| or |z2| below MASK_MARGIN in float64 (at most 10 %), and rows whose float64 1 - max p lies between 1e-9 and 1e-4, where
    float32 may or may not saturate (at most 4, all among the scaled rows)."""
    near, between, sat = ref["near_mask"][:P], ref["between"][:P], ref["saturated"][:P]
    assert near.sum() <= 0.1 * P, "%d of %d rows within %g of a relu kink" % (near.sum(), P, MASK_MARGIN)
    assert ref["between"].sum() <= 4 and not ref["between"][:N - SCALED].any()
    rows = ~near & ~between & ~sat
    assert not rows[N - SCALED:].any()          # test_egl_host.SEEDS: every scaled row saturates or is left out
    return rows, sat & ~near


@pytest.mark.parametrize("P", [1, 33, 70])
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=IDS)
def test_parity_with_the_float64_oracle_loop(gpu, shape, P):
    """EGL of the first P pairs against sum_c P(c) |g_c| of the oracle's float64 one-row gradients.  The tolerance is measured
    here: 4 x the largest relative error of the closed form in float32 NumPy on the same rows (the margin DESIGN.md §9 uses for
    the other gradient checks), floor 16 float32 ulps.  Saturated rows (float64
    1 - max p < 1e-9) must be exactly 0."""
    ref = reference(shape)
    head, _ = device_run(shape)
    got = head.expected_gradient_length_device(dev(ref["L"][:P]), dev(ref["R"][:P]))["egl"]
    assert got.shape == (P,) and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy().astype(np.float64)
    rows, sat = compared_rows(ref, P)
    r64 = ref["egl64"][:P]
    assert (r64[rows] > 0).all()
    fig = float((np.abs(ref["egl32"][:P].astype(np.float64) - r64)[rows] / r64[rows]).max())
    bound = np.maximum(4 * fig * r64, FLOOR_ULPS * np.spacing(r64.astype(np.float32)).astype(np.float64))
    err = np.abs(got - r64)
    rel = float((err[rows] / r64[rows]).max())
    print("%s P=%d: float32 NumPy figure %.3g, kernel %.3g relative (rows compared %d, saturated %d)" % (shape, P, fig, rel, rows.sum(), sat.sum()))
    assert (err[rows] <= bound[rows]).all(), "largest relative error %.3g, float32 NumPy %.3g" % (rel, fig)
    assert (got[sat] == 0.0).all()
    if P == N:
        assert sat.sum() >= 2


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=IDS)
def test_gradient_embedding(gpu, shape):
    """emb against the float64 outer product a2 x (p - onehot(yhat)) (= the oracle's gW3 for yhat, which the host test pins), and
    its squared row norms against |dz3|^2 |a2|^2.  The same tolerance rule, per ROW: the largest element error relative to the
    row's largest element — an element's own relative error is unbounded where a2[j] is a small difference of large sums, in
    NumPy's float32 as much as in the kernel's — measured on the float32 NumPy closed form, x 4, floor 16 float32 ulps."""
    ref = reference(shape)
    _, out = device_run(shape)
    od, h2 = shape[3], shape[2]
    got = out["emb"].cpu().numpy().astype(np.float64)
    assert got.shape == (N, od * h2)
    rows, sat = compared_rows(ref, N)
    r64 = ref["emb64"][rows]
    top = np.abs(r64).max(axis=1)
    assert (top > 0).all()
    rowerr = lambda a: np.abs(a - r64).max(axis=1) / top
    fig = float(rowerr(ref["emb32"][rows].astype(np.float64)).max())
    tol = max(4 * fig, FLOOR_ULPS * 2.0 ** -23)
    rel = float(rowerr(got[rows]).max())
    print("%s emb: float32 NumPy figure %.3g, kernel %.3g (row-wise)" % (shape, fig, rel))
    assert rel <= tol
    n64 = (r64 ** 2).sum(axis=1)                                   # = |p - onehot|^2 |a2|^2, float64
    nrel = float((np.abs((got[rows] ** 2).sum(axis=1) - n64) / n64).max())
    print("%s emb squared row norms: %.3g relative" % (shape, nrel))
    assert nrel <= tol
    assert (got[sat] == 0.0).all() and sat.sum() >= 2
    # the hypothesised label: class blocks carry p_c - [c = yhat], so the block of yhat is the negative one
    p = out["probs"].cpu().numpy()
    live = np.flatnonzero(rows)[:8]
    for i in live:
        blocks = got[i].reshape(od, h2)
        a2pos = np.abs(blocks).max(axis=0) > 0
        yhat = (int(p[i, 1] > p[i, 0]) if od == 2 else int(p[i, 0] > 0.5))
        if od == 2:
            assert (blocks[yhat][a2pos] < 0).all() and (blocks[1 - yhat][a2pos] > 0).all()
        else:
            assert ((blocks[0][a2pos] < 0) == bool(yhat)).all()


@pytest.mark.parametrize("shape", GPU_SHAPES, ids=IDS)
def test_bit_equalities(gpu, shape):
    ref = reference(shape)
    head, out = device_run(shape)
    L, R = dev(ref["L"]), dev(ref["R"])
    # the forward's probabilities
    assert same_bits(out["probs"], head.predict_device(L, R))
    # one output against all three
    assert same_bits(head.expected_gradient_length_device(L, R, want=("egl",))["egl"], out["egl"])
    assert same_bits(head.expected_gradient_length_device(L, R, want="emb")["emb"], out["emb"])
    # a pair scored alone against its row inside P = 70 (first and last row of a tile, the tail, a saturated row)
    for i in (0, 31, 32, 45, N - 1):
        alone = head.expected_gradient_length_device(L[i:i + 1].contiguous(), R[i:i + 1].contiguous(), want=ALL)
        for w in ALL:
            assert same_bits(alone[w], out[w][i:i + 1]), (w, i)
    # indexed (repeated, permuted) against materialised rows
    rng = np.random.RandomState(5)
    li = rng.randint(0, N, 90).astype(np.int32)
    ri = rng.permutation(np.concatenate([np.arange(N), rng.randint(0, N, 20)])).astype(np.int32)
    indexed = head.expected_gradient_length_device(L, R, dev(li), dev(ri), want=ALL)
    rows = head.expected_gradient_length_device(dev(ref["L"][li]), dev(ref["R"][ri]), want=ALL)
    for w in ALL:
        assert indexed[w].shape[0] == 90 and same_bits(indexed[w], rows[w]), w
    assert not np.array_equal(bits(indexed["egl"][:N]), bits(out["egl"]))          # not the identity pairing


def test_weights_that_move(gpu):
    """after one train_on_batch the EGL is that of a fresh head loaded with the new weights: the packed W2^T copy is re-derived"""
    shape = GPU_SHAPES[0]
    ref = reference(shape)
    head = make_head(shape, ref["ws"])
    L, R = dev(ref["L"]), dev(ref["R"])
    before = head.expected_gradient_length_device(L, R, want=ALL)                   # allocates and fills the W2^T copy
    y = O.to_categorical(np.random.RandomState(2).randint(0, 2, 16))
    head.train_on_batch([ref["L"][:16], ref["R"][:16]], y)
    after = head.expected_gradient_length_device(L, R, want=ALL)
    fresh = make_head(shape, head.get_weights()).expected_gradient_length_device(L, R, want=ALL)
    for w in ALL:
        assert same_bits(after[w], fresh[w]), w
    assert not np.array_equal(bits(after["egl"]), bits(before["egl"]))


def _committee(D, members=3):
    from a_link_amd import committee, siamese
    nets = []
    for m in range(members):
        net = siamese.SiameseNetwork((D,), "e%d" % m, 0.1, seed=60 + m)
        ws = net.siamese_net.get_weights()
        ws[4] = ws[4] * np.float32(40.0)                                            # probabilities spread over (0, 1)
        net.siamese_net.set_weights(ws)
        nets.append(net)
    return committee.Bagging(nets, [])


def test_committee_mean_and_ranked_batch(gpu):
    from a_link_amd import batch as B, density as Dn
    D, n_pairs, k = 64, 300, 12
    rng = np.random.RandomState(9)
    bag = _committee(D)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    L, R = dev(unit(rng.randn(40, D))), dev(unit(rng.randn(9, D)))
    li, ri = dev(rng.randint(0, 40, n_pairs).astype(np.int32)), dev(rng.randint(0, 9, n_pairs).astype(np.int32))
    got = bag.egl_indexed(L, R, li, ri)
    e = [m.siamese_net.expected_gradient_length_device(L, R, li, ri)["egl"] for m in bag.models]
    e = [t.cpu().numpy() for t in e]                                                # the mean formed in float32 NumPy: an IEEE division
    assert np.array_equal(bits(got), (((e[0] + e[1]) + e[2]) / np.float32(3.0)).view(np.uint32))
    assert same_bits(bag.egl_indexed([L] * 3, [R] * 3, li, ri), got)                # one matrix per member
    assert same_bits(bag._indexed_utility(L, R, li, ri, "egl"), got)
    labeled = (L[li[:5].long()] - R[ri[:5].long()]).abs().contiguous()
    idx, sc = bag.ranked_batch_indexed(L, R, li, ri, labeled, k, kind="egl")
    idx2, sc2 = B.ranked_batch_device((L, R, li, ri), bag.egl_indexed(L, R, li, ri), labeled, k)
    assert torch.equal(idx, idx2) and same_bits(sc, sc2) and idx.numel() == k
    cold, _ = bag.ranked_batch_cold_indexed(L, R, li, ri, k, kind="egl")
    assert cold.numel() == k and len(set(cold.tolist())) == k
    weighted = Dn.density_weighted(got, bag.density_indexed(L, R, li, ri))
    assert weighted.shape == got.shape and bool(torch.isfinite(weighted).all())
    # the 128-wide gradient embeddings as the rows of a ranked batch (the pieces BADGE would need)
    out = bag.models[0].siamese_net.expected_gradient_length_device(L, R, li, ri, want=("egl", "emb"))
    assert out["emb"].shape == (n_pairs, 128)
    pick, _ = B.ranked_batch_device(out["emb"], out["egl"], out["emb"][:8].contiguous(), 5)
    assert pick.numel() == 5 and int(pick.min()) >= 0 and len(set(pick.tolist())) == 5
    with pytest.raises(ValueError, match="egl"):
        bag._indexed_utility(L, R, li, ri, "margin")

    class Host(object):
        siamese_net = None
    from a_link_amd import committee
    with pytest.raises(TypeError, match="DenseHead"):
        committee.Bagging([Host()], []).egl_indexed(L, R, li, ri)


def test_sampler_on_the_device(gpu):
    from a_link_amd import egl, uncertainty
    shape = GPU_SHAPES[0]
    ref = reference(shape)
    head, out = device_run(shape)
    L, R = dev(ref["L"]), dev(ref["R"])
    idx, inst = egl.egl_sampling(head, [L, R], n_instances=5)
    assert np.array_equal(idx, uncertainty.multi_argmax(out["egl"].cpu().numpy(), n_instances=5))
    assert torch.equal(inst[0], L[torch.from_numpy(idx).cuda()])
    host_idx, _ = egl.egl_sampling(head, [ref["L"], ref["R"]], n_instances=5)         # NumPy inputs: the host form, through get_weights()
    assert np.array_equal(host_idx, uncertainty.multi_argmax(egl.expected_gradient_length(head.get_weights(), [ref["L"], ref["R"]]), 5))


def test_python_refusals(gpu):
    from a_link_amd import egl
    shape = GPU_SHAPES[0]
    ref = reference(shape)
    head, _ = device_run(shape)
    L, R = dev(ref["L"]), dev(ref["R"])
    li = dev(np.arange(4, dtype=np.int32))
    run = head.expected_gradient_length_device
    for args, kw, text in (((L.cpu(), R), {}, "CUDA tensor"), ((L, ref["R"]), {}, "CUDA tensor"), ((L.double(), R), {}, "float32"),
                           ((L, R[:, :32].contiguous()), {}, "D = 32"), ((L[:, :32].contiguous(), R), {}, "D = 32"),
                           ((L[:10], R), {}, "differ in rows"), ((L, R, li), {}, "come together"),
                           ((L, R, li.long(), li), {}, "int32"), ((L, R, li.cpu(), li), {}, "CUDA"),
                           ((L, R, li, li[:3]), {}, "differ in length"), ((L, R, li + N, li), {}, "outside"),
                           ((L, R, li, li - 1), {}, "outside"), ((L, R), dict(want=("egl", "norm")), "norm"), ((L, R), dict(want=()), "unknown")):
        with pytest.raises(ValueError, match=text):
            run(*args, **kw)
    quant = make_head(shape, ref["ws"])
    quant.set_compute_dtype("bf16")
    with pytest.raises(ValueError, match="bf16"):
        quant.expected_gradient_length_device(L, R)
    with pytest.raises(TypeError):
        egl.egl_sampling(object(), [L, R])
    empty = run(L[:0], R[:0], want=ALL)
    assert empty["egl"].shape == (0,) and empty["emb"].shape == (0, shape[3] * shape[2])


def test_c_entry_refusals_launch_nothing(gpu):
    shape = GPU_SHAPES[0]
    ref = reference(shape)
    head, _ = device_run(shape)
    lib = gpu.load()
    L, R = dev(ref["L"]), dev(ref["R"])
    egl_, probs, emb = (torch.full(s, -7.0, device="cuda") for s in ((N,), (N, shape[3]), (N, shape[3] * shape[2])))
    st = gpu.current_stream(0)
    quant = make_head(shape, ref["ws"])
    quant.set_compute_dtype("bf16")

    def call(h=head.h, l=L, r=R, P=N, accumulate=0, e=egl_, p=probs, m=emb):
        return lib.alink_head_egl(h, gpu.ptr(l), gpu.ptr(r), None, None, P, accumulate, 0.0, gpu.ptr(e), gpu.ptr(p), gpu.ptr(m), st)
    for kw, text in ((dict(h=None), "NULL head"), (dict(l=None), "NULL feature table"), (dict(r=None), "NULL feature table"),
                     (dict(e=None, p=None, m=None), "all NULL"), (dict(P=-1), "negative"), (dict(accumulate=1, e=None), "accumulate"),
                     (dict(h=quant.h), "bf16")):
        assert call(**kw) == -1, kw                                                  # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(P=-1), "alink_head_egl")
    assert call(P=0) == 0                                                            # nothing to do is not an error
    torch.cuda.synchronize()
    for t in (egl_, probs, emb):
        assert bool((t == -7.0).all())                                               # a refused call launches nothing
    assert call(p=None, m=None) == 0                                                 # one output is enough
    torch.cuda.synchronize()
    assert bool((egl_ != -7.0).all()) and bool((probs == -7.0).all())
