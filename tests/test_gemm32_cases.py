"""CPU: the exact-f32 GEMM cases (tests/gemm32_cases.py) are what they claim.  The GPU test demands BIT equality with a float64
reference; that is a fair demand only if the reference itself is a float32 value that any order of float32 sums reaches.  For
every exact case: the float64 reference survives a round trip through float32; a float32 CPU computation of the same operation
(torch matmul / conv2d / its autograd, whose summation order is not the kernel's) equals it exactly; and the sum of |products|
plus the epilogue terms stays below 2^24 units of the smallest operand step, so no partial sum in ANY order can round.  A GPU
mismatch is then the kernel's."""
import pytest
import torch

import gemm32_cases as G


@pytest.mark.parametrize("group", sorted(G.GROUPS))
def test_exact_cases_need_no_rounding(group):
    for c in G.GROUPS[group]:
        ref = c.reference()
        assert ref.shape == (c.M, c.N) and ref.dtype == torch.float64, c.name
        assert torch.isfinite(ref).all(), c.name
        assert torch.equal(ref.float().double(), ref), "%s: the reference is no float32 value" % c.name
        f32 = G.epilogue(c, G.linear(c, torch.float32), torch.float32)
        assert f32.dtype == torch.float32 and torch.equal(f32.double(), ref), "%s: float32 on the CPU differs from float64" % c.name
        units = float(G.magnitude(c).max()) / G.unit(c)
        assert units < 2 ** 24, "%s: %g units of %g: a partial sum could round" % (c.name, units, G.unit(c))
        assert c.K <= 8192, c.name


def test_operands_are_the_small_integers_the_argument_needs():
    for c in G.EXACT_CASES:
        pre = c.geom["prescale"]
        for t in c.a_parts:
            v = t[~torch.isnan(t)]
            assert torch.equal(v, v.round()), c.name
            lo, hi = (0, 255) if pre else (-8, 8)
            assert v.min() >= lo and v.max() <= hi, c.name
            assert v.numel() < 64 or (v != 0).float().mean() > 0.8, c.name
        v = c.b_store[~torch.isnan(c.b_store)]
        assert torch.equal(v, v.round()) and v.abs().max() <= 8 and (v.numel() < 64 or (v != 0).float().mean() > 0.8), c.name
        for t in (c.bias, c.resid, c.oldc):
            assert t is None or torch.equal(t, t.round()), c.name
        if c.alpha is not None:
            assert set(c.alpha.tolist()) <= {0.25, 0.5}, c.name
        if c.act is not None:                                    # zeros of both signs, positives and negatives
            bits = c.act.view(torch.int32)
            assert (bits == 0).any() and (bits == -2 ** 31).any() and (c.act > 0).any() and (c.act < 0).any(), c.name


def test_instantiation_table_is_complete():
    """all 48 (amode, bmode, tile, stage, vec) combinations have a case written for them, whose stated form agrees with the
    launcher's documented rules"""
    assert len(G.ALL_FORMS) == 48 and sorted(G.INSTANTIATIONS) == sorted(G.ALL_FORMS)
    for form, name in G.INSTANTIATIONS.items():
        c = G.BY_NAME[name]
        assert c.form == form, (name, c.form, form)
    reached = {}
    for c in G.EXACT_CASES:
        assert tuple(c.expect) == G.form_of(c), "%s: written for %s, the documented rules give %s" % (c.name, c.expect, G.form_of(c))
        reached.setdefault(c.form, []).append(c.name)
    assert sorted(reached) == sorted(G.ALL_FORMS)
    assert min(len(v) for v in reached.values()) >= 2            # no instantiation hangs on its pin case alone


def test_the_issue_s_shapes_are_all_there():
    names = set(G.BY_NAME)
    for pair in ("row-row", "row-colt", "col-row"):
        for M in (1, 63, 65, 129):
            for N in (8, 32, 33, 100):
                for K in (4, 17, 28, 64, 65, 200):
                    assert "plain-%s-%dx%dx%d" % (pair, M, N, K) in names
    splits = {c.split[0] for c in G.GROUPS["slabs/fixed"] if c.M * c.N == 33}
    assert {2, 8, 9, 17} <= splits
    assert any(c.max_split >= 1 and c.split and c.split[0] > 1 for c in G.GROUPS["slabs/planned"])
    for tag in list(G.EPILOGUE_TERMS) + ["all"]:
        cs = G.GROUPS["epilogue/" + tag]
        assert any(c.split is None and c.max_split == 1 for c in cs) and any(c.max_split == 0 and c.splitk > 1 for c in cs)


def test_real_cases_cover_every_mode_pair():
    cs = G.real_cases()
    assert {(c.amode, c.bmode) for c in cs} == set(G.PAIRS)
    assert all(c.K <= 640 and not c.exact for c in cs)
