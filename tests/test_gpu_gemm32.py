"""Direct parity of the exact-f32 GEMM (a-link_amd/csrc/sgemm.hip) through alink_gemm32_ex: every operand mode, tile form, stage
depth, loader form and split, each launch against a float64 CPU reference that does not share the kernel's indexing
(tests/gemm32_cases.py).

EXACT cases hold small integers, so every product and every partial sum in any order is a float32 value (checked without a
device by tests/test_gemm32_cases.py) and the kernel's result must EQUAL the reference: no tolerance.  A wrong tap, a missed zero
pad, a dropped slab, a swapped epilogue step or a mis-wrapped pixel walk changes an integer.  Every launch writes into a
NaN-filled output with guard rows behind M, guard columns behind N (ldc > N, unsplit) and NaN margins around it, all of which
must still be NaN; operands sit between NaN margins and their row padding is NaN, so a value fetched from outside an operand
and used shows up as NaN.  Every case asserts the (tile, stage, loader form) the entry REPORTS against the form it was written
for; gemm32_cases.INSTANTIATIONS names the case that pins each of the 48 kernel instantiations.

REAL cases (randn, K <= 640) are held to the worst case of a float32 accumulation,
|err| <= (K + splitk + 8) 2^-24 (sum|a||b| + |bias| + |resid| + |old C|): a lower-precision matrix instruction, which integers
cannot catch, would miss it more than ten times over."""
import ctypes as C

import pytest
import torch

import gemm32_cases as G

pytestmark = pytest.mark.gpu

MARGIN = 1024          # NaN floats before and behind every device buffer handed to the kernel
GUARD_ROWS = 3
NAN = float("nan")


def _place(t, off=0):
    """t's values at `off` floats past a 16-byte aligned address, NaN margins around; returns (buffer, address)"""
    flat = t.contiguous().view(-1)
    d = torch.full((2 * MARGIN + 4 + flat.numel(),), NAN, device="cuda")
    assert d.data_ptr() % 16 == 0
    d[MARGIN + off:MARGIN + off + flat.numel()] = flat.cuda()
    return d, d.data_ptr() + 4 * (MARGIN + off)


def _pitched(t, ld):
    s = torch.full((t.shape[0], ld), NAN)
    s[:, :t.shape[1]] = t
    return s


def launch(gpu, c, ws_floats=None, workspace=True):
    """one alink_gemm32_ex call; returns (rc, report, output incl. guards (M + GUARD_ROWS, ldc), everything around it)"""
    lib = gpu.load()
    keep, d = [], gpu.Gemm32Desc()

    def put(t, off=0, pitch=None):
        if t is None:
            return None
        buf, addr = _place(t if pitch is None else _pitched(t, pitch), off)
        keep.append(buf)
        return addr

    d.A = put(c.a_parts[0], c.a_off)
    d.A2 = put(c.a_parts[1]) if len(c.a_parts) > 1 else None
    d.a_split = c.a_split
    d.B = put(c.b_store, c.b_off)
    d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.amode, d.bmode = c.M, c.N, c.K, c.lda, c.ldb, c.ldc, c.amode, c.bmode
    for k, v in c.geom.items():
        setattr(d, k, v)
    d.bias, d.alpha = put(c.bias), put(c.alpha)
    d.act, d.resid = put(c.act, pitch=c.ldc), put(c.resid, pitch=c.ldc)
    d.relu, d.accumulate, d.splitk, d.kper, d.force_bk = c.relu, c.accumulate, c.splitk, c.kper, c.force_bk
    rows = c.M + GUARD_ROWS
    out = torch.full((rows, c.ldc), NAN)
    if c.oldc is not None:
        out[:c.M, :c.N] = c.oldc
    cbuf, d.C = _place(out)
    need = max(c.max_split, c.splitk, 1) * c.M * c.ldc
    ws = torch.full((need + 64,), NAN, device="cuda")            # NaN: a slab element that is summed without having been written shows
    report = (C.c_int * 5)(-7, -7, -7, -7, -7)
    rc = lib.alink_gemm32_ex(C.byref(d), c.max_split, C.c_void_p(ws.data_ptr()) if workspace else None,
                             need if ws_floats is None else ws_floats, report, None)
    torch.cuda.synchronize()
    whole = cbuf.cpu()
    body = whole[MARGIN:MARGIN + rows * c.ldc].view(rows, c.ldc)
    around = torch.cat([whole[:MARGIN], whole[MARGIN + rows * c.ldc:]])
    del keep
    return rc, list(report), body, around


def run(gpu, c):
    """a launch that must succeed in the form the case was written for; returns (result (M, N), report) after the guard checks"""
    rc, report, body, around = launch(gpu, c)
    gpu.check(rc, "alink_gemm32_ex %s" % c.name)
    assert tuple(report[:3]) == tuple(c.expect), "%s: ran (tile, stage, vec) = %s, written for %s" % (c.name, report[:3], c.expect)
    if c.split is not None:
        assert tuple(report[3:]) == tuple(c.split), "%s: ran (splitk, kper) = %s, written for %s" % (c.name, report[3:], c.split)
    elif c.max_split == 1:
        assert report[3] == 1, (c.name, report)
    assert torch.isnan(around).all(), "%s: wrote outside the output buffer" % c.name
    assert torch.isnan(body[c.M:]).all(), "%s: wrote a guard row" % c.name
    assert torch.isnan(body[:, c.N:]).all(), "%s: wrote a guard column" % c.name
    return body[:c.M, :c.N].contiguous(), report


def check_exact(gpu, c):
    got, report = run(gpu, c)
    ref = c.reference().float()
    if not torch.equal(got, ref):
        bad = (got != ref) | torch.isnan(got)
        at = bad.nonzero()[0].tolist()
        raise AssertionError("%s (report %s): %d of %d outputs differ, first at %s: got %r, reference %r" % (
            c.name, report, int(bad.sum()), bad.numel(), at, float(got[at[0], at[1]]), float(ref[at[0], at[1]])))
    return got


@pytest.mark.parametrize("group", sorted(G.GROUPS))
def test_exact(gpu, group):
    wrong = []
    for c in G.GROUPS[group]:
        try:
            check_exact(gpu, c)
        except AssertionError as e:                              # (a failed CALL is no AssertionError: it ends the test at once)
            wrong.append(str(e))
    assert not wrong, "%d of %d cases:\n%s" % (len(wrong), len(G.GROUPS[group]), "\n".join(wrong))


def test_every_instantiation_has_its_case():
    """the table of which case pins which (amode, bmode, tile, stage, vec): complete, and each pin case is in a group above,
    where its form is asserted from the entry's report"""
    assert sorted(G.INSTANTIATIONS) == sorted(G.ALL_FORMS) and len(G.ALL_FORMS) == 48
    for form, name in G.INSTANTIATIONS.items():
        assert G.BY_NAME[name].form == form


# ---- requests the entry must refuse: an error code, a message, all five report fields -1, and not one element written ----------
def _refusals():
    big = lambda c: setattr(c, "ldc", c.N + 3) or c
    as_row = lambda c: (setattr(c, "amode", G.A_ROW), setattr(c, "lda", c.K), setattr(c, "a_parts", [torch.ones(c.M, c.K)])) and c
    return {
        "split-with-ldc-not-N": (big(G.plain("refuse-ldc", G.A_ROW, G.B_ROW, 65, 33, 200, **G.fixed(4, 64))), {}),
        "flip-with-ci-6": (G.dgrad("refuse-ci6", 2, 5, 7, 6, 32, 1), {}),
        "flip-with-a-row": (as_row(G.dgrad("refuse-flip-row", 2, 5, 7, 4, 32, 1)), {}),
        "a-col-with-b-colt": (G.plain("refuse-col-colt", G.A_COL, G.B_COLT, 68, 32, 28), {}),
        "kper-24": (G.plain("refuse-kper24", G.A_ROW, G.B_ROW, 65, 33, 40, **G.fixed(2, 24)), {}),
        "force-bk-32": (G.plain("refuse-bk32", G.A_ROW, G.B_ROW, 65, 33, 200, force_bk=32), {}),
        "split-without-workspace": (G.plain("refuse-no-ws", G.A_ROW, G.B_ROW, 65, 33, 200, **G.fixed(4, 64)), dict(workspace=False)),
        "workspace-too-small": (G.plain("refuse-small-ws", G.A_ROW, G.B_ROW, 65, 33, 200, **G.fixed(4, 64)),
                                dict(ws_floats=4 * 65 * 33 - 1)),
        "planned-workspace-too-small": (G.plain("refuse-small-ws-planned", G.A_ROW, G.B_ROW, 65, 33, 520, max_split=8, ldc=None),
                                        dict(ws_floats=3 * 65 * 33 - 1)),
    }


@pytest.mark.parametrize("what", sorted(_refusals()))
def test_refused(gpu, what):
    c, kw = _refusals()[what]
    rc, report, body, around = launch(gpu, c, **kw)
    assert rc != 0, "%s was launched (report %s)" % (what, report)
    assert gpu.load().alink_last_error(), what
    assert report == [-1] * 5, (what, report)
    assert torch.isnan(body).all() and torch.isnan(around).all(), "%s: refused, yet the output was written" % what


def test_refusals_would_run_once_mended(gpu):
    """the refused requests are refused for the stated reason alone: the same operands with that one field mended run and match"""
    c, _ = _refusals()["split-with-ldc-not-N"]
    c.ldc = c.N
    check_exact(gpu, c)
    c, _ = _refusals()["workspace-too-small"]
    check_exact(gpu, c)
    c, _ = _refusals()["kper-24"]
    c.kper, c.splitk, c.expect = 32, 2, (64, 16, 0)
    check_exact(gpu, c)


# ---- real-valued operands against the float32 accumulation bound -----------------------------------------------------------------
_REAL = {c.name: c for c in G.real_cases()}


@pytest.mark.parametrize("name", sorted(_REAL))
def test_real_valued_within_the_f32_accumulation_bound(gpu, name):
    c = _REAL[name]
    got, report = run(gpu, c)
    assert torch.isfinite(got).all(), name
    err = (got.double() - c.reference()).abs()
    bound = G.error_bound(c, report[3])
    print("%s report %s: max err %.3g, max err / bound %.3g" % (name, report, float(err.max()), float((err / bound).max())))
    assert (err <= bound).all(), "%s: err / bound up to %.3g" % (name, float((err / bound).max()))


# ---- batch invariance under one caller-fixed plan (alink_smallres_score_pairs relies on it) ---------------------------------------
def _sub_plain(big, off, rows, plan):
    a = big.a_parts[0][off:off + rows].contiguous()
    return G.Case("%s-rows%d" % (big.name, off), "plain", big.amode, big.bmode, rows, big.N, big.K, [a], big.b_store, lda=big.lda,
                  ldb=big.ldb, exact=False, bias=big.bias, relu=big.relu, **plan)


def _sub_conv(big, off, rows, plan):                             # one output pixel per image: rows are images
    x = big.a_parts[0][off:off + rows].contiguous()
    return G.Case("%s-rows%d" % (big.name, off), "conv", big.amode, big.bmode, rows, big.N, big.K, [x], big.b_store, ldb=big.ldb,
                  geom=big.geom, exact=False, bias=big.bias, relu=big.relu, **plan)


@pytest.mark.parametrize("mode", ["row-row", "conv-row"])
def test_rows_do_not_depend_on_the_batch(gpu, mode):
    """the rows of an M = 7 problem have the same BITS as the same rows inside an M = 200 problem, at row offsets 0 and 150,
    under one fixed (splitk, kper, force_bk)"""
    if mode == "row-row":
        plans = [G.fixed(3, 256, 64), G.fixed(7, 96, 64), G.fixed(2, 320, 16)]      # deep, 16 by kper, 16 by the caller
        make = lambda plan: G.plain("batch-row-row", G.A_ROW, G.B_ROW, 200, 100, 640, exact=False, terms=("bias", "relu"), **plan)
        sub = _sub_plain
    else:
        plans = [G.fixed(2, 64, 64), G.fixed(2, 48, 64), G.fixed(1, 128, 16)]
        make = lambda plan: G.conv("batch-conv-row", 200, 3, 3, 8, 40, 3, 1, 0, exact=False, terms=("bias", "relu"), **plan)
        sub = _sub_conv
    for plan in plans:
        big = make(plan)
        assert big.M == 200
        full, rep_full = run(gpu, big)
        err = (full.double() - big.reference()).abs()
        assert (err <= G.error_bound(big, rep_full[3])).all()
        for off in (0, 150):
            small = sub(big, off, 7, plan)
            part, rep = run(gpu, small)
            assert rep == rep_full, (rep, rep_full)
            assert torch.equal(part.view(torch.int32), full[off:off + 7].contiguous().view(torch.int32)), \
                "%s plan %s: rows %d.. differ between M = 7 and M = 200" % (mode, plan, off)
