"""GPU: committee disagreement on device (alink_committee_disagreement, select.hip) — values against the float64 formulas of
modAL.disagreement restated with scipy.stats.entropy, the two bit-equalities the header promises, the multiset rule of vote
entropy, edges, and the sharded-pool path that asks for the new kinds."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.stats import entropy

pytestmark = pytest.mark.gpu

MS, CS = (1, 2, 3, 5, 8), (2, 3, 7, 32)
ATOL = 2e-6             # what tests/test_gpu_pool.py grants the entropy kind; holds for C <= 7 (see test_values_against_float64)
ATOL_C32 = 2.74e-6      # C = 32: twice the float32 emulation's own error there (1.37e-6)
OUTPUTS = ("vote_entropy", "consensus_entropy", "max_disagreement", "consensus", "votes")


def _atol(c):
    return ATOL if c <= 7 else ATOL_C32


def _member_probs(M, P, Cn, seed):
    """softmaxes of seeded normal logits, per-row scale drawn from {0.1, 1, 5, 30}: near-uniform rows and saturated rows
    whose small entries are float32 denormals"""
    rng = np.random.RandomState(seed)
    scale = rng.choice([0.1, 1.0, 5.0, 30.0], size=(1, P, 1))
    z = rng.randn(M, P, Cn) * scale
    e = np.exp(z - z.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).astype(np.float32)


def _reference(p):
    """float64 modAL formulas on (M, P, C) float32 probabilities -> votes (P, M), vote entropy, consensus entropy, max KL"""
    p64 = p.astype(np.float64)
    M, _, Cn = p.shape
    votes = p.argmax(axis=2).T
    p_vote = np.stack([(votes == c).sum(axis=1) for c in range(Cn)], axis=1) / float(M)
    consensus = p64.mean(axis=0)
    kl = np.stack([entropy(p64[m], qk=consensus, axis=1) for m in range(M)], axis=1)
    return {"votes": votes, "vote_entropy": entropy(p_vote, axis=1), "consensus_entropy": entropy(consensus, axis=1),
            "max_disagreement": kl.max(axis=1), "consensus": consensus}


_CASES = {}


def _case(M, Cn, P=4096):
    """inputs and their float64 reference, made once per shape and shared (read-only) among the tests"""
    key = (M, Cn, P)
    if key not in _CASES:
        p = _member_probs(M, P, Cn, 1000 * M + Cn)
        _CASES[key] = (p, _reference(p))
    return _CASES[key]


def _check_against_reference(got, ref, Cn):
    assert np.array_equal(got["votes"].cpu().numpy(), ref["votes"])
    errs = {}
    for name in ("vote_entropy", "consensus_entropy", "max_disagreement"):
        g = got[name].cpu().numpy()
        assert np.isfinite(g).all(), name
        errs[name] = float(np.abs(g.astype(np.float64) - ref[name]).max())
    print("C=%d  max |device - float64|: %s" % (Cn, "  ".join("%s %.2e" % kv for kv in sorted(errs.items()))))
    for name, err in errs.items():
        assert err <= _atol(Cn), (name, err)
    assert np.isfinite(got["consensus"].cpu().numpy()).all()
    # M - 1 float32 additions and one division, each within half an ulp (2^-24 relative; a denormal's half ulp is 7e-46)
    M = ref["votes"].shape[1]
    np.testing.assert_allclose(got["consensus"].cpu().numpy(), ref["consensus"], rtol=M * 2.0 ** -24, atol=1e-45)
    return errs


@pytest.mark.parametrize("Cn", CS)
@pytest.mark.parametrize("M", MS)
def test_values_against_float64(gpu, M, Cn):
    """P = 4096, all five outputs in one call.  The bound: a float32 NumPy emulation of the kernel's operation order, on
    these same inputs (host CPU), differs from the float64 formulas by at most
        C = 2: 3.2e-7    C = 3: 3.7e-7    C = 7: 7.2e-7    C = 32: 1.37e-6      (the largest of the three measures, M <= 8)
    so atol = 2e-6 (the entropy kind's tolerance in tests/test_gpu_pool.py) stands for C <= 7, and C = 32, whose emulation
    exceeds 1e-6, gets twice its own emulation error: 2.74e-6.  M = 2, C = 7 is the case a ratio formed against the divided
    mean fails: a denormal probability over a mean that underflowed to 0 gives inf."""
    from a_link_amd import disagreement as D
    p, ref = _case(M, Cn)
    if (M, Cn) == (2, 7):
        assert ((p > 0) & (p < np.finfo(np.float32).tiny)).any()          # the denormal entries are there
    got = D.score_members_device(torch.from_numpy(p).cuda(), want=OUTPUTS)
    assert got["votes"].dtype == torch.int32 and got["votes"].shape == (p.shape[1], M)
    _check_against_reference(got, ref, Cn)
    # a list of separate (P, C) tensors is the same call
    again = D.score_members_device([torch.from_numpy(p[m].copy()).cuda() for m in range(M)], want=OUTPUTS)
    for name in OUTPUTS:
        assert torch.equal(again[name], got[name]), name


def _three_heads(d_in=64):
    from a_link_amd.head import DenseHead
    heads = []
    for m in range(3):
        h = DenseHead(d_in, lr=0.1, seed=20 + m)
        ws = h.get_weights()
        ws[4] = ws[4] * np.float32(40.0)            # probabilities spread over (0, 1), not 0.5 +- 0.02
        h.set_weights(ws)
        heads.append(h)
    return heads


def test_consensus_and_its_entropy_bit_equal_the_mean_path(gpu):
    """consensus == committee_predict_device (alink_committee_forward / _multi) and consensus_entropy == score_device(that
    mean, "entropy"), bit for bit: shared matrices, and one matrix pair per member gathered through index lists"""
    from a_link_amd import disagreement as D, head as H, uncertainty as U
    heads = _three_heads()
    rng = np.random.RandomState(7)
    L, R = rng.randn(1000, 64).astype(np.float32), rng.randn(1000, 64).astype(np.float32)
    Ls = [torch.from_numpy(rng.randn(50, 64).astype(np.float32)).cuda() for _ in heads]
    Rs = [torch.from_numpy(rng.randn(9, 64).astype(np.float32)).cuda() for _ in heads]
    li = torch.from_numpy(rng.randint(0, 50, 777).astype(np.int32)).cuda()
    ri = torch.from_numpy(rng.randint(0, 9, 777).astype(np.int32)).cuda()
    for args in ((torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()), (Ls, Rs, li, ri)):
        mean = H.committee_predict_device(heads, *args)
        members = H.committee_member_probs_device(heads, *args)
        assert members.shape == (3,) + tuple(mean.shape)
        for m, h in enumerate(heads):                # slab m is that member's own predict_device
            own = (args[0][m], args[1][m], li, ri) if len(args) == 4 else args
            assert torch.equal(members[m], h.predict_device(*own))
        got = D.score_members_device(members, want=("consensus", "consensus_entropy"))
        spread = mean[:, 0].cpu().numpy()
        assert spread.min() < 0.3 and spread.max() > 0.7
        assert torch.equal(got["consensus"], mean)
        assert torch.equal(got["consensus_entropy"], U.score_device(mean, "entropy"))
    from a_link_amd.head import DenseHead
    with pytest.raises(TypeError):
        H.committee_member_probs_device([DenseHead(64, seed=1, out_dim=1)], torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda())


def test_vote_entropy_is_a_function_of_the_multiset_of_counts(gpu):
    """M = 5, C = 7: permuting the class columns of every member permutes the counts among the classes — vote entropy must
    not move by a bit, or top-k's ties would follow float noise instead of the lower index"""
    from a_link_amd import disagreement as D
    p, ref = _case(5, 7)
    base = D.score_members_device(torch.from_numpy(p).cuda(), want=("vote_entropy", "votes"))
    counts = np.stack([(ref["votes"] == c).sum(axis=1) for c in range(7)], axis=1)
    assert (np.sort(counts, axis=1)[:, -3] > 0).any()                  # rows with three non-zero terms: where order could matter
    for seed in range(3):
        perm = np.random.RandomState(seed).permutation(7)
        q = np.ascontiguousarray(p[:, :, perm])
        got = D.score_members_device(torch.from_numpy(q).cuda(), want=("vote_entropy", "votes"))
        assert np.array_equal(got["votes"].cpu().numpy(), q.argmax(axis=2).T)
        assert torch.equal(got["vote_entropy"], base["vote_entropy"])


@pytest.mark.parametrize("P", [1, 255, 256, 257, 70001])
def test_sizes_and_each_output_alone(gpu, P):
    """sizes around the 256-thread workgroup and one of several hundred workgroups; C = 7 runs the one-float loads, C = 2 the
    two-float loads (C = 32 in test_values_against_float64: four).  Every output asked for alone equals the all-outputs call."""
    from a_link_amd import disagreement as D
    for M, Cn in ((3, 7), (3, 2)):
        p, ref = _case(M, Cn, P)
        pd = torch.from_numpy(p).cuda()
        every = D.score_members_device(pd, want=OUTPUTS)
        _check_against_reference(every, ref, Cn)
        for name in OUTPUTS:
            alone = D.score_members_device(pd, want=(name,))
            assert list(alone) == [name] and torch.equal(alone[name], every[name]), name


def test_slabs_off_the_vector_alignment(gpu):
    """members whose rows start 4 bytes off an 8- or 16-byte boundary take the one-float path: same bits"""
    from a_link_amd import disagreement as D
    for M, Cn in ((3, 2), (2, 32)):
        p, _ = _case(M, Cn)
        P = p.shape[1]
        want = D.score_members_device(torch.from_numpy(p).cuda(), want=OUTPUTS)
        shifted = []
        for m in range(M):
            flat = torch.empty(P * Cn + 1, dtype=torch.float32, device="cuda")
            view = flat[1:].view(P, Cn)
            view.copy_(torch.from_numpy(p[m]))
            assert view.is_contiguous() and view.data_ptr() % 8 == 4
            shifted.append(view)
        got = D.score_members_device(shifted, want=OUTPUTS)
        for name in OUTPUTS:
            assert torch.equal(got[name], want[name]), name


def test_more_pairs_than_one_grid_sweep(gpu):
    """the grid stops at 65,536 workgroups of 256 and strides: one pair beyond 2^24 runs the second sweep.  One member, so
    the consensus (p / 1) must return the input bit for bit in every row, and its entropy must equal alink_score's."""
    from a_link_amd import disagreement as D, uncertainty as U
    P = 65536 * 256 + 1
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    p = torch.rand((P, 2), generator=g, device="cuda", dtype=torch.float32)
    got = D.score_members_device([p], want=("consensus", "consensus_entropy", "vote_entropy"))
    assert torch.equal(got["consensus"], p)
    assert torch.equal(got["consensus_entropy"], U.score_device(p, "entropy"))
    assert not bool(got["vote_entropy"].any())                         # one member: one class holds every vote


def _raw_call(lib, members, M, P, Cn, outs):
    arr = (C.c_void_p * max(1, len(members)))(*[t.data_ptr() for t in members])
    return lib.alink_committee_disagreement(arr, M, P, Cn, *[C.c_void_p(o.data_ptr()) if o is not None else None for o in outs],
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_empty_pool_and_rejected_shapes(gpu):
    lib = gpu.load()
    p = torch.from_numpy(_case(2, 3, 256)[0]).cuda()
    sentinel = torch.full((256,), -7.0, device="cuda")
    outs = [sentinel, None, None, None, None]
    assert _raw_call(lib, [p[0], p[1]], 2, 0, 3, outs) == 0             # P == 0: success, nothing written
    torch.cuda.synchronize()
    assert bool((sentinel == -7.0).all())
    for M, Cn in ((0, 3), (65, 3), (2, 1), (2, 33)):
        members = [p[0]] * max(M, 1)
        assert _raw_call(lib, members, M, 256, Cn, outs) == -1          # ALINK_EINVAL
        msg = lib.alink_last_error().decode()
        assert ("n_members=%d" % M in msg) if M in (0, 65) else ("C=%d" % Cn in msg), msg
    torch.cuda.synchronize()
    assert bool((sentinel == -7.0).all())
    from a_link_amd import disagreement as D
    with pytest.raises(gpu.AlinkError):
        D.score_members_device(torch.zeros((2, 4, 1), device="cuda"))
    with pytest.raises(ValueError):
        D.score_members_device(p, want=("entropy",))
    # and the limits themselves run: 64 members, 32 classes (the emulation's own error at this shape: 1.13e-6, inside C = 32's 1.37e-6)
    q, ref = _case(64, 32, 64)
    _check_against_reference(D.score_members_device(torch.from_numpy(q).cuda(), want=OUTPUTS), ref, 32)


def test_a_nan_never_wins_the_vote(gpu):
    from a_link_amd import disagreement as D
    p = _case(3, 7, 256)[0].copy()
    rows = np.arange(256)
    cols = rows % 7                                                     # every column, the first one included
    p[1, rows, cols] = np.nan
    votes = D.score_members_device(torch.from_numpy(p).cuda(), want=("votes",))["votes"].cpu().numpy()
    assert (votes[:, 1] != cols).all()
    assert np.array_equal(votes[:, 1], np.nanargmax(p[1], axis=1))     # the first maximum of what is left
    assert np.array_equal(votes[:, [0, 2]], p[[0, 2]].argmax(axis=2).T)


def test_pool_topk_by_disagreement_and_bagging(gpu):
    """distributed.committee_pool_topk with the new kinds on one rank (no process group): three backbones — four residual
    units on 32 x 32 images, the network of smoke(), so that the case takes seconds — embed n = 24 pool and g = 4 gallery images,
    k = 16 of the 96 pairs.  The selection is exact (ties to the lower index) on the device's own scores, and those scores
    are the float64 formulas of the members' own predict_device outputs within the tolerance above."""
    from a_link_amd import committee, disagreement as D, distributed as Dist, siamese, weights as W
    from a_link_amd.backbone import IRBackbone
    size, n, g, k = (32, 32), 24, 4, 16
    rng = np.random.default_rng(2)
    pool = torch.from_numpy(rng.integers(0, 256, (n,) + size + (3,), dtype=np.uint8)).cuda()
    gal = torch.from_numpy(rng.integers(0, 256, (g,) + size + (3,), dtype=np.uint8)).cuda()
    bbs, nets = [], []
    for m in range(3):
        bbs.append(IRBackbone(W.synthetic_ir_params((1, 2, 1, 1), size=size, seed=3 + m), image_size=size, max_batch=32))
        net = siamese.SiameseNetwork((512,), "c%d" % m, 0.1, seed=30 + m)
        ws = net.siamese_net.get_weights()
        ws[4] = ws[4] * np.float32(40.0)
        net.siamese_net.set_weights(ws)
        nets.append(net)
    heads = [net.siamese_net for net in nets]
    Ep, Eg = [bb.embed_device(pool) for bb in bbs], [bb.embed_device(gal) for bb in bbs]
    li = torch.arange(n, dtype=torch.int32, device="cuda").repeat_interleave(g)
    ri = torch.arange(g, dtype=torch.int32, device="cuda").repeat(n)
    members = np.stack([h.predict_device(Ep[m], Eg[m], li, ri).cpu().numpy() for m, h in enumerate(heads)])     # (3, 96, 2)
    ref = _reference(members)
    assert len(set(np.round(ref["vote_entropy"], 6))) > 1               # the members do split their votes somewhere
    bag = committee.Bagging(nets, [])
    for kind in ("vote_entropy", "max_disagreement", "consensus_entropy"):
        scores = bag.disagreement_indexed(Ep, Eg, li, ri, kind=kind)
        s = scores.cpu().numpy()
        assert s.shape == (n * g,) and np.isfinite(s).all()
        err = float(np.abs(s.astype(np.float64) - ref[kind]).max())
        print("pool path, %s: max |device - float64| %.2e" % (kind, err))
        assert err <= ATOL, (kind, err)
        vals, idx = Dist.committee_pool_topk(bbs, heads, pool, gal, k, shard_offset=5, kind=kind)
        want = np.lexsort((np.arange(n * g), -s))[:k]                  # ties -> lower index
        assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), want + 5 * g)
        assert np.array_equal(vals.cpu().numpy(), s[want])
    # Bagging.disagreement on host arrays is the indexed form on the gathered rows
    Lh, Rh = Ep[0][li.long()].cpu().numpy(), Eg[0][ri.long()].cpu().numpy()
    for kind in ("vote_entropy", "max_disagreement"):
        host = bag.disagreement([Lh, Rh], kind=kind)
        assert isinstance(host, np.ndarray)
        assert np.array_equal(host, bag.disagreement_indexed(Ep[0], Eg[0], li, ri, kind=kind).cpu().numpy())
    # the kinds that were there keep their path and their answer
    v0, i0 = Dist.committee_pool_topk(bbs, heads, pool, gal, k, shard_offset=0)
    v1, i1 = Dist.committee_pool_topk(bbs, heads, pool, gal, k, shard_offset=0, kind="entropy")
    assert torch.equal(v0, v1) and torch.equal(i0, i1)
