"""GPU: ALFA-Mix's feature mix on device (alink_head_feature_mix, alfamix.hip) — the mixed rows against the float64 host under a
tolerance measured in the same test, flips against the host's outside a measured band, bit equalities (the forward's
probabilities on the rows and on the mixed rows, indexed against materialised rows, a pair alone against the pair in a pool, one
output against all four, one anchor against three), weights that move, the batch rule against the host's, the committee form, and
every refusal."""
import functools

import numpy as np
import pytest
import torch

from oracle import siamese_head as O
from test_alfamix_host import FLIPPING, IDS, N, SHAPES, case
from test_egl_host import make_case

pytestmark = pytest.mark.gpu

FLOOR_ULPS = 16                                    # MFMA's k-ordered chain and NumPy's BLAS order the sums differently
MASK_MARGIN = 2e-5                                 # |z1| or |z2| below it: a relu mask may legitimately flip in float32
ALL = ("probs", "flip", "mixed_probs", "mixed")
EPS = {s: FLIPPING.get(s, (0.5, 0))[0] for s in SHAPES}    # (8, 128, 32, 2) flips nothing up to 0.5: the arithmetic alone


def restate32(ws, L, R, anchors, eps):
    """the rule of alfamix.feature_mix in float32 NumPy -> (mixed (N, A, D), margin (N, A)), both float32"""
    f = np.float32
    W1, b1, W2, b2, W3, b3 = [np.asarray(w, f) for w in ws]
    d = np.abs(L - R)
    z1 = d @ W1 + b1
    z2 = np.maximum(z1, 0) @ W2 + b2
    z3 = np.maximum(z2, 0) @ W3 + b3
    od = z3.shape[1]
    yhat = (z3[:, 1] > z3[:, 0]) if od == 2 else (z3[:, 0] > 0)
    wd = W3[:, 0] - W3[:, 1] if od == 2 else W3[:, 0]
    q = (((wd[None, :] * (z2 > 0)) @ W2.T) * (z1 > 0)) @ W1.T
    sign = np.where(yhat, f(1), f(-1)) if od == 2 else np.where(yhat, f(-1), f(1))
    g = sign[:, None] * q
    G = np.sqrt((g * g).sum(axis=1, dtype=f))
    mixed, margin = np.empty((len(d), len(anchors), d.shape[1]), f), np.empty((len(d), len(anchors)), f)
    for a, an in enumerate(np.asarray(anchors, f)):
        z = an[None, :] - d
        Z = np.sqrt((z * z).sum(axis=1, dtype=f))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = (f(eps) * Z / G)[:, None] * g
            delta = np.minimum(np.maximum(t, np.minimum(z, 0)), np.maximum(z, 0))
        delta = np.where(((G != 0) & np.isfinite(G) & np.isfinite(Z))[:, None], delta, f(0))
        mixed[:, a] = d + delta
        m3 = np.maximum(np.maximum(mixed[:, a] @ W1 + b1, 0) @ W2 + b2, 0) @ W3 + b3
        margin[:, a] = (np.where(yhat, m3[:, 1] - m3[:, 0], m3[:, 0] - m3[:, 1]) if od == 2 else np.where(yhat, m3[:, 0], -m3[:, 0]))
    return mixed, margin


@functools.lru_cache(maxsize=None)
def reference(shape):
    """computed once per shape and left unchanged: the inputs, the float64 host, the float32 restatement, the rows near a kink"""
    from a_link_amd import alfamix
    ws, L, R, Ld, y, anchors = case(shape)
    eps = EPS[shape]
    out = alfamix.feature_mix(ws, [L, R], anchors, eps=eps)
    _, (d, z1, a1, z2, a2) = O.forward(ws, L, R, dtype=np.float64, cache=True)
    near_mask = np.minimum(np.abs(z1).min(axis=1), np.abs(z2).min(axis=1)) < MASK_MARGIN
    mixed32, margin32 = restate32(ws, L, R, anchors, eps)
    ref = dict(ws=ws, L=L, R=R, anchors=anchors, eps=eps, d=d, near_mask=near_mask, mixed32=mixed32, margin32=margin32, **out)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    # the conditions this shape is here for, in the float64 reference
    flip = out["flip"]
    if shape in FLIPPING:
        assert (flip != 0).sum() == FLIPPING[shape][1]
        assert all(0 < (flip >> a & 1).sum() < N for a in range(3))
    else:
        assert not flip.any()
    return ref


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
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def device_run(shape):
    """all four outputs of the whole 70-pair case, once per shape -> (head, {name: tensor})"""
    ref = reference(shape)
    head = make_head(shape, ref["ws"])
    return head, head.feature_mix_device(dev(ref["L"]), dev(ref["R"]), ref["anchors"], eps=ref["eps"], want=ALL)


def argmax_rule(p):
    return (p[..., 1] > p[..., 0]) if p.shape[-1] == 2 else (p[..., 0] > 0.5)


@pytest.mark.parametrize("P", [1, 33, 70])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_the_forward_and_the_float64_host(gpu, shape, P):
    """The first P pairs.  probs and mixed_probs are the forward's bits on the rows and on the mixed rows (which are >= 0, so
    |x - 0| = x): the flips are what a caller who materialised the mixed rows would get.  The mixed rows against the float64
    host: error of a row = max_e |delta_dev - delta_64| / (eps Z); tolerance = 4 x the same error of the float32 NumPy
    restatement on the same rows (the margin DESIGN.md §9 uses for the other gradient checks), floor 16 float32 ulps; left out
    are only rows with a float64 |z1| or |z2| below 2e-5 (at most 10 %).  Flips equal the host's on every row whose float64
    mixed margin lies outside a band of 4 x the restatement's margin error relative to max(1, |m|); at most 2 rows inside."""
    ref = reference(shape)
    head, _ = device_run(shape)
    eps, A, D = ref["eps"], 3, shape[0]
    L, R = dev(ref["L"][:P]), dev(ref["R"][:P])
    out = head.feature_mix_device(L, R, ref["anchors"], eps=eps, want=ALL)
    assert out["probs"].shape == (P, shape[3]) and out["flip"].shape == (P,) and out["flip"].dtype == torch.uint8
    assert out["mixed_probs"].shape == (P, A, shape[3]) and out["mixed"].shape == (P, A, D) and out["mixed"].is_cuda
    assert same_bits(out["probs"], head.predict_device(L, R))
    assert bool((out["mixed"] >= 0).all())
    zeros = torch.zeros_like(L)
    for a in range(A):
        assert same_bits(out["mixed_probs"][:, a].contiguous(), head.predict_device(out["mixed"][:, a].contiguous(), zeros)), a
    probs, mp, flip = out["probs"].cpu().numpy(), out["mixed_probs"].cpu().numpy(), out["flip"].cpu().numpy()
    flipped = argmax_rule(mp) != argmax_rule(probs)[:, None]                          # (P, A)
    assert np.array_equal(flip, (flipped * (1 << np.arange(A))).sum(axis=1).astype(np.uint8))
    # ---- the mixed rows against the float64 host ----
    near = ref["near_mask"][:P]
    assert near.sum() <= 0.1 * P, "%d of %d rows within %g of a relu kink" % (near.sum(), P, MASK_MARGIN)
    rows = ~near
    d64 = ref["d"][:P]
    delta64 = ref["mixed"][:P] - d64[:, None, :]
    z = ref["anchors"].astype(np.float64)[None, :, :] - d64[:, None, :]
    scale = eps * np.sqrt((z * z).sum(axis=2))                                        # eps Z, (P, A)
    assert (scale > 0).all()
    d32 = np.abs(ref["L"][:P] - ref["R"][:P]).astype(np.float64)                      # the float32 row both float32 forms start from
    rowerr = lambda mixed: (np.abs((mixed.astype(np.float64) - d32[:, None, :]) - delta64).max(axis=2) / scale)[rows]
    fig = float(rowerr(ref["mixed32"][:P]).max()) if rows.any() else 0.0
    tol = max(4 * fig, FLOOR_ULPS * 2.0 ** -23)
    got = float(rowerr(out["mixed"].cpu().numpy()).max()) if rows.any() else 0.0
    print("%s P=%d eps=%g: mixed rows: float32 NumPy figure %.3g, kernel %.3g, tolerance %.3g (rows compared %d)"
          % (shape, P, eps, fig, got, tol, rows.sum()))
    # ---- flips against the float64 host's, outside the band ----
    m64 = ref["margin"][:P]
    mfig = (np.abs(ref["margin32"][:P].astype(np.float64) - m64) / np.maximum(1, np.abs(m64)))[rows]     # measured on the same rows
    mfig = float(mfig.max()) if rows.any() else 0.0
    inside = np.abs(m64) <= 4 * mfig * np.maximum(1, np.abs(m64))
    host = (ref["flip"][:P, None] >> np.arange(A) & 1).astype(bool)
    print("%s P=%d: margin figure %.3g, smallest |m| %.3g, rows inside the band %d, flips %d (host %d)"
          % (shape, P, mfig, np.abs(m64).min(), inside.any(axis=1).sum(), flipped.sum(), host.sum()))
    assert got <= tol, "largest row error %.3g, float32 NumPy %.3g" % (got, fig)
    assert inside.any(axis=1).sum() <= 2
    assert np.array_equal(flipped[~inside], host[~inside])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bit_equalities(gpu, shape):
    ref = reference(shape)
    head, out = device_run(shape)
    eps, anchors = ref["eps"], dev(ref["anchors"])
    L, R = dev(ref["L"]), dev(ref["R"])
    run = lambda l, r, li=None, ri=None, want=ALL, an=anchors: head.feature_mix_device(l, r, an, li, ri, eps=eps, want=want)
    # one output against all four
    for w in ALL:
        assert same_bits(run(L, R, want=w)[w], out[w]), w
    # a pair alone against its row inside P = 70 (first and last row of a tile, the tail, a scaled row)
    for i in (0, 31, 32, 45, N - 1):
        alone = run(L[i:i + 1].contiguous(), R[i:i + 1].contiguous())
        for w in ALL:
            assert same_bits(alone[w], out[w][i:i + 1]), (w, i)
    # indexed (repeated, permuted) against materialised rows
    rng = np.random.RandomState(5)
    li = rng.randint(0, N, 90).astype(np.int32)
    ri = rng.permutation(np.concatenate([np.arange(N), rng.randint(0, N, 20)])).astype(np.int32)
    indexed = run(L, R, dev(li), dev(ri))
    rows = run(dev(ref["L"][li]), dev(ref["R"][ri]))
    for w in ALL:
        assert indexed[w].shape[0] == 90 and same_bits(indexed[w], rows[w]), w
    assert not np.array_equal(bits(indexed["mixed"][:N]), bits(out["mixed"]))      # not the identity pairing
    # one anchor against column 0 of three; the second alone against column 1
    for a in (0, 1):
        one = run(L, R, an=anchors[a:a + 1].contiguous())
        assert same_bits(one["mixed"][:, 0], out["mixed"][:, a]) and same_bits(one["mixed_probs"][:, 0], out["mixed_probs"][:, a])
        assert torch.equal(one["flip"], out["flip"] >> a & 1) and same_bits(one["probs"], out["probs"])


def test_weights_that_move(gpu):
    """after set_weights the mix is that of a fresh head loaded with the new weights: the packed W1^T copy follows"""
    shape = SHAPES[0]
    ref = reference(shape)
    head = make_head(shape, ref["ws"])
    L, R = dev(ref["L"]), dev(ref["R"])
    before = head.feature_mix_device(L, R, ref["anchors"], eps=0.1, want=ALL)      # allocates and fills the W1^T copy
    ws2, _, _ = make_case(*shape, seed=4)
    head.set_weights(ws2)
    after = head.feature_mix_device(L, R, ref["anchors"], eps=0.1, want=ALL)
    fresh = make_head(shape, ws2).feature_mix_device(L, R, ref["anchors"], eps=0.1, want=ALL)
    for w in ALL:
        assert same_bits(after[w], fresh[w]), w
    assert not np.array_equal(bits(after["mixed"]), bits(before["mixed"]))
    y = O.to_categorical(np.random.RandomState(2).randint(0, 2, 16))               # and after a train step
    head.train_on_batch([ref["L"][:16], ref["R"][:16]], y)
    stepped = head.feature_mix_device(L, R, ref["anchors"], eps=0.1, want=ALL)
    fresh = make_head(shape, head.get_weights()).feature_mix_device(L, R, ref["anchors"], eps=0.1, want=ALL)
    for w in ALL:
        assert same_bits(stepped[w], fresh[w]), w


def integer_pool():
    """200 pairs of small-integer features (D = 16), a head on them and anchors: k-means on such rows rounds nowhere, so the
    device's picks are the host's"""
    rng = np.random.RandomState(11)
    shape = (16, 128, 32, 2)
    ws = O.init_weights(*shape[:3], seed=5, out_dim=2)
    ws[4] = ws[4] * np.float32(8.0)
    L = rng.randint(0, 5, (200, 16)).astype(np.float32)
    R = rng.randint(0, 5, (200, 16)).astype(np.float32)
    from a_link_amd import alfamix
    lab = np.abs(L[:30] - R[30:60])
    y = alfamix._argmax(alfamix.feature_mix(ws, [lab, np.zeros_like(lab)], np.zeros((1, 16), np.float32), eps=0.0)["probs"])
    return shape, ws, L, R, alfamix.class_anchors(lab, y)


def test_select_device_gives_the_hosts_picks(gpu):
    from a_link_amd import alfamix
    shape, ws, L, R, anchors = integer_pool()
    head = make_head(shape, ws)
    dL, dR = dev(L), dev(R)
    info = head.feature_mix_device(dL, dR, anchors, eps=0.2)
    flip, probs = info["flip"].cpu().numpy(), info["probs"].cpu().numpy()
    c = int((flip != 0).sum())
    print("integer pool: %d of 200 candidates" % c)
    assert 8 < c < 200
    rows = np.abs(L - R)
    ar = torch.arange(200, dtype=torch.int32, device="cuda")
    for kw in (dict(), dict(exclude=np.flatnonzero(flip)[:c - 5])):                # the k-means route; 5 candidates left: the fill
        want = alfamix.select(rows, flip, probs, 8, iters=3, random_state=4, **kw)
        got = alfamix.select_device((dL, dR, ar, ar), info["flip"], info["probs"], 8, iters=3, seed=4, **kw)
        assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(got.cpu().numpy(), want), (kw, got, want)
        got = alfamix.select_device((dL - dR).abs(), info["flip"], info["probs"], 8, iters=3, seed=4, **kw)     # a row table
        assert np.array_equal(got.cpu().numpy(), want)
    picks, info2 = alfamix.alfamix_device(head, dL, dR, None, None, anchors, 8, eps=0.2, iters=3, seed=4)
    assert np.array_equal(picks.cpu().numpy(), alfamix.select(rows, flip, probs, 8, iters=3, random_state=4))
    assert torch.equal(info2["flip"], info["flip"])
    for n in (1, 8, 50, 200, 500):
        p = alfamix.alfamix_device(head, dL, dR, ar, ar, anchors, n, eps=0.2, iters=2, seed=0)[0].cpu().numpy()
        assert len(p) == min(n, 200) and len(set(p.tolist())) == len(p) and p.min() >= 0 and p.max() < 200, n


def test_the_fill_case_and_the_sampler(gpu):
    from a_link_amd import alfamix
    shape = (128, 384, 64, 1)
    ws, L, R, Ld, y, anchors = case(shape)
    assert (alfamix.feature_mix(ws, [L, R], anchors, eps=0.2)["flip"] != 0).sum() == 3          # 3 candidates of 70, n = 8
    head = make_head(shape, ws)
    dL, dR = dev(L), dev(R)
    info = head.feature_mix_device(dL, dR, anchors, eps=0.2)
    flip, probs = info["flip"].cpu().numpy(), info["probs"].cpu().numpy()
    assert 0 < (flip != 0).sum() < 8
    want = alfamix.select(np.abs(L - R), flip, probs, 8)
    picks, _ = alfamix.alfamix_device(head, dL, dR, None, None, anchors, 8, eps=0.2)
    assert np.array_equal(picks.cpu().numpy(), want) and len(set(want.tolist())) == 8
    assert np.array_equal(want[:(flip != 0).sum()], np.flatnonzero(flip))
    # the sampler: CUDA input goes to the device form, NumPy input through get_weights() to the host form

    class Learner(object):
        estimator = None
        siamese_net = head
        X_training, y_training = [Ld, np.zeros_like(Ld)], y
    a2 = alfamix.class_anchors(Learner.X_training, y)
    idx, inst = alfamix.alfamix_sampling(Learner(), [dL, dR], n_instances=8, eps=0.2)
    p2, _ = alfamix.alfamix_device(head, dL, dR, None, None, a2, 8, eps=0.2)
    assert np.array_equal(idx, p2.cpu().numpy()) and torch.equal(inst[0], dL[torch.from_numpy(idx).cuda()])
    host_idx, _ = alfamix.alfamix_sampling(Learner(), [L, R], n_instances=8, eps=0.2)
    assert np.array_equal(host_idx, alfamix.alfamix(head.get_weights(), [L, R], a2, 8, eps=0.2)[0])


def test_committee_ors_the_members_masks_and_spares_the_labelled(gpu):
    from a_link_amd import alfamix, committee, siamese
    D, n_pairs, k = 64, 300, 12
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
    y = rng.randint(0, 2, 30)
    y[:2] = (0, 1)
    picks, info = bag.alfamix_indexed(L, R, li, ri, labelled, y, k, eps=0.3, iters=3, seed=1)
    picks = picks.cpu().numpy()
    assert len(picks) == k and len(set(picks.tolist())) == k and not set(picks.tolist()) & set(labelled.tolist())
    take = torch.from_numpy(labelled).cuda()
    rows = (L[li[take].long()] - R[ri[take].long()]).abs().cpu().numpy()
    assert np.array_equal(info["anchors"], alfamix.class_anchors(rows, y))
    masks = [m.siamese_net.feature_mix_device(L, R, info["anchors"], li, ri, eps=0.3, want="flip")["flip"] for m in bag.models]
    assert torch.equal(info["flip"], masks[0] | masks[1])
    assert same_bits(info["probs"], bag.predict_indexed(L, R, li, ri))
    want = alfamix.select((L[li.long()] - R[ri.long()]).abs().cpu().numpy(), info["flip"].cpu().numpy(), info["probs"].cpu().numpy(), k,
                          exclude=labelled)
    assert set(want.tolist()).isdisjoint(labelled.tolist()) and len(want) == k
    with pytest.raises(ValueError, match="one feature space|one left"):
        bag.alfamix_indexed([L, L], [R, R], li, ri, labelled, y, k)
    with pytest.raises(ValueError, match="labelled"):
        bag.alfamix_indexed(L, R, li, ri, [], [], k)

    class Host(object):
        siamese_net = None
    with pytest.raises(TypeError, match="DenseHead"):
        committee.Bagging([Host()], []).alfamix_indexed(L, R, li, ri, labelled, y, k)


def test_python_refusals(gpu):
    shape = SHAPES[0]
    ref = reference(shape)
    head, _ = device_run(shape)
    L, R, an = dev(ref["L"]), dev(ref["R"]), ref["anchors"]
    li = dev(np.arange(4, dtype=np.int32))
    run = head.feature_mix_device
    for args, kw, text in (((L.cpu(), R, an), {}, "CUDA tensor"), ((L.double(), R, an), {}, "float32"),
                           ((L, R[:, :32].contiguous(), an), {}, "D = 32"), ((L[:10], R, an), {}, "differ in rows"),
                           ((L, R, an, li), {}, "come together"), ((L, R, an, li.long(), li), {}, "int32"),
                           ((L, R, an, li, li[:3]), {}, "differ in length"), ((L, R, an, li + N, li), {}, "outside"),
                           ((L, R, an), dict(want=("flip", "delta")), "delta"), ((L, R, an), dict(want=()), "unknown"),
                           ((L, R, an[:, :32]), {}, "anchors"), ((L, R, np.zeros((9, shape[0]), np.float32)), {}, "anchors"),
                           ((L, R, dev(an)[:0]), {}, "anchors"), ((L, R, an), dict(eps=-1.0), "eps"),
                           ((L, R, an), dict(eps=float("inf")), "eps")):
        with pytest.raises(ValueError, match=text):
            run(*args, **kw)
    quant = make_head(shape, ref["ws"])
    quant.set_compute_dtype("bf16")
    with pytest.raises(ValueError, match="bf16"):
        quant.feature_mix_device(L, R, an)
    wide = make_head((520, 256, 64, 2))
    with pytest.raises(ValueError, match="512"):
        wide.feature_mix_device(torch.zeros(4, 520, device="cuda"), torch.zeros(4, 520, device="cuda"), np.zeros((1, 520), np.float32))
    empty = run(L[:0], R[:0], an, want=ALL)
    assert empty["flip"].shape == (0,) and empty["mixed"].shape == (0, 3, shape[0])


def test_c_entry_refusals_launch_nothing(gpu):
    # (a D off a multiple of 8 and an h1 outside {128, 256, 384, 512} are refused too, but alink_head_create_ex makes no such head)
    shape = SHAPES[0]
    ref = reference(shape)
    head, _ = device_run(shape)
    lib = gpu.load()
    L, R, an = dev(ref["L"]), dev(ref["R"]), dev(ref["anchors"])
    D, od = shape[0], shape[3]
    probs, mp, mixed = (torch.full(s, -7.0, device="cuda") for s in ((N, od), (N, 3, od), (N, 3, D)))
    flip = torch.full((N,), 0xA5, dtype=torch.uint8, device="cuda")
    st = gpu.current_stream(0)
    quant = make_head(shape, ref["ws"])
    quant.set_compute_dtype("bf16")
    wide = make_head((520, 256, 64, 2))

    def call(h=head.h, l=L, r=R, P=N, a=an, A=3, eps=0.1, p=probs, f=flip, m=mp, x=mixed):
        return lib.alink_head_feature_mix(h, gpu.ptr(l), gpu.ptr(r), None, None, P, gpu.ptr(a), A, eps, gpu.ptr(p), gpu.ptr(f),
                                          gpu.ptr(m), gpu.ptr(x), st)
    for kw, text in ((dict(h=None), "NULL head"), (dict(l=None), "NULL feature table"), (dict(r=None), "NULL feature table"),
                     (dict(a=None), "NULL anchors"), (dict(p=None, f=None, m=None, x=None), "all NULL"), (dict(P=-1), "negative"),
                     (dict(P=(1 << 29) - 31), "2^29"), (dict(A=0), "anchors"), (dict(A=9), "anchors"), (dict(eps=-0.5), "eps"),
                     (dict(eps=float("nan")), "eps"), (dict(eps=float("inf")), "eps"), (dict(h=quant.h), "bf16"),
                     (dict(h=wide.h), "D=520")):
        assert call(**kw) == -1, kw                                                  # ALINK_EINVAL
        assert text in lib.alink_last_error().decode(), (kw, lib.alink_last_error())
    with pytest.raises(gpu.AlinkError):
        gpu.check(call(A=9), "alink_head_feature_mix")
    assert call(P=0) == 0                                                            # nothing to do is not an error
    torch.cuda.synchronize()
    for t in (probs, mp, mixed):
        assert bool((t == -7.0).all())                                               # a refused call launches nothing
    assert bool((flip == 0xA5).all())
    assert call(p=None, m=None, x=None) == 0                                         # one output is enough
    torch.cuda.synchronize()
    assert bool((flip < 8).all()) and bool((probs == -7.0).all()) and bool((mixed == -7.0).all())
