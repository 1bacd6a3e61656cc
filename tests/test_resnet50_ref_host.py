"""CPU: the one-op references of tests/resnet50_ref.py are the network, their tolerances hold for a float32 device in all
three types, and they catch every mutant.

Four things, none of which needs a GPU:
  (a) chained without rounding, at 197 x 228 and 224 x 224, the op references reproduce oracle/vgg_resnet50.forward in float64
      to 5e-12 of the feature scale (the figure tests/test_gpu_resnet50_grad.py uses for its restatement; measured 3e-16 and
      6e-16).  The chain runs
      with the oracle's epsilon, the double 1e-3; the device folds with the float32 1e-3f (4.75e-11 larger), which moves the
      features by 4.1e-11 of their scale — measured and printed, far below anything a type here resolves;
  (b) a stand-in device — torch's float32 convolution of the same operands, the residual added in float32, the result stored
      in T or as an f16 pair under the scale calibration would choose, fed op by op with its own outputs as the GPU test feeds
      the device's — stays within every tolerance.  Measured at 197 x 228, one image, largest err / tol:
          bf16   conv / stem 0.93, average pool 0.03, max-pool exact
          f16    conv / stem 0.39, average pool 0.03, max-pool exact
          f16x2  conv / stem 0.14, average pool 0.12, max-pool exact (hi + lo has at most 22 bits: float32 holds it)
      and the stem alone on raw pixels 0.85 / 0.30 / 0.07;
  (c) every mutant of the reference leaves the tolerance in more than 1 % of the outputs of every image at every op it applies
      to.  Measured smallest share over the ops a mutant applies to (bf16; f16 and f16x2 differ in the third digit):
          bias rolled by one channel            0.50      adjacent output channels swapped      0.62
          3x3 taps transposed                   0.44      ReLU dropped                          0.43
          post_relu dropped on increase         0.18      residual dropped                      0.43
          residual from the unit input          0.84      stride-2 1x1 sampling odd positions   0.53
          max-pool windows one pixel late       0.69      average dividing by 64                0.88
          stem pad before and after swapped     0.67      stem channels not flipped (raw)       0.70
          stem means by source channel (raw)    0.58
      (the average by 64: the other 12 % are channels whose 7 x 7 map is all zero.)  None of the mutants is confined to a
      border ring — a swapped pad shifts the whole map — so none is judged on a ring.  "Residual from the unit input" reads the
      first unit's residual from the unit's input buffer as the kernel would, flat [pixel][Cout] memory; it applies to conv3_1,
      conv4_1 and conv5_1 (conv2_1's input is smaller than its projection);
  (d) the literal kernel tables of tests/test_gpu_resnet50_layers.py follow the choosers' rules as resnet50_ref restates them.
"""
import numpy as np
import pytest
import torch

import resnet50_ref as R

torch.set_num_threads(min(16, torch.get_num_threads()))
H, W, N = 197, 228, 1
SHARE = 0.01


@pytest.fixture(scope="module")
def params():
    return R.draw_params(11)


@pytest.fixture(scope="module")
def images():
    return np.random.default_rng(5).standard_normal((N, H, W, 3)).astype(np.float32)


def _chain_unrounded(params, x, eps):
    outs = {}
    for i, op in enumerate(R.OPS):
        A = R.stem_pixels(x, None, True) if op.src is None else outs[op.src]
        outs[i] = R.op_ref(params, None, i, A, None if op.res is None else outs[op.res], eps)[0]
    return outs[len(R.OPS) - 1].reshape(x.shape[0], -1).numpy()


@pytest.mark.parametrize("size", [(197, 228), (224, 224)])
def test_chained_references_are_the_oracle(params, size):
    from oracle import vgg_resnet50 as O
    x = np.random.default_rng(6).standard_normal((1,) + size + (3,)).astype(np.float32)
    want = O.forward(params, x, dtype=torch.float64)
    got = _chain_unrounded(params, x, O.BN_EPS)
    scale = np.abs(want).max()
    d = np.abs(got - want).max() / scale
    d32 = np.abs(_chain_unrounded(params, x, R.EPS32) - want).max() / scale
    print("%s: chained references against the float64 oracle: %.2e of the feature scale %.3g (with the float32 epsilon: %.2e)"
          % (size, d, scale, d32))
    assert got.shape == want.shape == (1, 2048)
    assert d <= 5e-12, d
    assert d32 <= 1e-9, d32


def _beyond(mut, ref, tol):
    """per image: the share of outputs where the mutant leaves the tolerance around the reference"""
    return ((mut - ref).abs() > tol).double().mean(dim=(1, 2, 3))


class _Shares(object):
    def __init__(self, dt):
        self.dt, self.least = dt, {}

    def add(self, what, opname, share):
        print("    %-40s %-24s share %s" % (what, opname, ["%.3f" % v for v in share.tolist()]))
        self.least[what] = min(self.least.get(what, 1.0), float(share.min()))
        assert (share > SHARE).all(), (self.dt, opname, what, share)

    def report(self):
        for what, v in self.least.items():
            print("%s mutant %-40s smallest share %.3f" % (self.dt, what, v))


@pytest.mark.parametrize("dt", R.TYPES)
def test_standin_within_tolerance_and_mutants_beyond(params, images, dt):
    x2 = dt == "f16x2"
    outs, exps, worst, shares = {}, {}, {"conv": 0.0, "avgpool": 0.0, "maxpool": 0.0}, _Shares(dt)
    for i, op in enumerate(R.OPS):
        A = R.stem_pixels(images, dt, True) if op.src is None else outs[op.src]
        Rs = None if op.res is None else outs[op.res]
        ref, Wt, bias = R.op_ref(params, dt, i, A, Rs)
        if op.kind == "maxpool":
            e = exps[op.src]
            exps[i] = e
            if x2:                                         # one float32 rounding of hi + lo, then the pair again
                hi, lo = R.split_pair((ref * 2.0 ** e).float())
                got = (hi.double() + lo.double()) * 2.0 ** -e
                tol = R.maxpool_x2_tolerance(ref * 2.0 ** e) * 2.0 ** -e
                w = R.worst(got, ref, tol)
            else:                                          # a maximum of 16-bit values is one of them: nothing to round
                got, tol, w = ref, torch.zeros_like(ref), 0.0
            worst["maxpool"] = max(worst["maxpool"], w)
            print("%s %s stand-in err/tol %.3f" % (dt, op.name, w))
            assert w <= 1.0, (op.name, w)
            shares.add("max-pool windows one pixel late", op.name, _beyond(R.maxpool_late(A), ref, tol))
        elif op.kind == "avgpool":
            got, tol = R.avgpool_standin(A), R.avgpool_tolerance(A)
            w = R.worst(got, ref, tol)
            worst["avgpool"] = w
            print("%s %s stand-in err/tol %.3f" % (dt, op.name, w))
            assert w <= 1.0, (op.name, w)
            shares.add("average dividing by 64", op.name, _beyond(R.avgpool_by_64(A), ref, tol))
        else:
            tol = R.conv_tolerance(op, dt, ref, A, Wt, bias, Rs)
            y = R.conv_pre(op, A.float(), Wt.float(), bias.float(), None if Rs is None else Rs.float())
            got, exps[i] = R.store(torch.relu(y) if (op.relu or op.post_relu) else y, dt)
            w = R.worst(got, ref, tol)
            worst["conv"] = max(worst["conv"], w)
            print("%s %s %dx%d stand-in err/tol %.3f" % (dt, op.name, ref.shape[2], ref.shape[3], w))
            assert w <= 1.0, (op.name, w)
            for what, (applies, mutant) in R.CONV_MUTANTS.items():
                if applies(op):
                    shares.add(what, op.name, _beyond(mutant(op, A, Wt, bias, Rs), ref, tol))
            if op.kind == "stem":
                pad = R.stem_pad_swapped(A.shape[2], A.shape[3])
                assert pad != R.stem_pad(A.shape[2], A.shape[3])          # 228 wide: 2 / 3
                shares.add("stem pad before and after swapped", op.name, _beyond(R.conv_ref(op, A, Wt, bias, None, pad), ref, tol))
            X = None if op.unit_in is None else outs[op.unit_in]
            if Rs is not None and R.resid_from_unit_input_applies(op, Rs, X):
                assert not op.name.startswith("conv2_1")
                shares.add("residual from the unit input", op.name, _beyond(R.resid_from_unit_input(op, A, Wt, bias, Rs, X), ref, tol))
        outs[i] = got
    print("%s: largest stand-in err / tol: conv and stem %.3f, average pool %.3f, max-pool %.3f" % (
        dt, worst["conv"], worst["avgpool"], worst["maxpool"]))
    shares.report()
    assert set(shares.least) == set(R.CONV_MUTANTS) | {"max-pool windows one pixel late", "average dividing by 64",
                                                        "stem pad before and after swapped", "residual from the unit input"}


@pytest.mark.parametrize("dt", R.TYPES)
def test_stem_mutants_on_raw_pixels(params, dt):
    x = np.random.default_rng(7).integers(0, 256, (N, H, W, 3)).astype(np.float32)
    op = R.OPS[0]
    Wt, b = R.weights_t(params, op.name, dt)
    A = R.stem_pixels(x, dt, False)
    ref = R.conv_ref(op, A, Wt, b)
    tol = R.conv_tolerance(op, dt, ref, A, Wt, b)
    w = R.worst(R.conv_standin(op, A, Wt, b, None, dt), ref, tol)
    print("%s stem on raw pixels: stand-in err/tol %.3f" % (dt, w))
    assert w <= 1.0
    # the flip and the means are the oracle's own preprocessing, exactly, before the type rounds them
    from oracle import vgg_resnet50 as O
    assert torch.equal(R.stem_pixels(x, None, False), R.nchw(torch.from_numpy(O.preprocess_input_v2(x)).double()))
    assert torch.equal(A, R.stem_pixels(O.preprocess_input_v2(x), dt, True))
    for what, kw in (("stem channels not flipped", dict(flip=False)), ("stem means indexed by source channel", dict(means_bgr=False))):
        share = _beyond(R.conv_ref(op, R.stem_pixels(x, dt, False, **kw), Wt, b), ref, tol)
        print("%s %s: share %s" % (dt, what, share.tolist()))
        assert (share > SHARE).all(), (what, share)


def test_gpu_tables_follow_the_rules():
    """the literal per-case kernel tables of tests/test_gpu_resnet50_layers.py against direct_variant_tiles / linear_variant_x2 /
    served_form as resnet50_ref restates them"""
    import test_gpu_resnet50_layers as G
    for case, c in G.CASES.items():
        for dt in R.TYPES:
            want = R.expected_table(c["size"][0], c["size"][1], c["mb"], dt, 1600 if c["lat"] is None else c["lat"])
            assert G.table_rows(case, dt) == want, (case, dt)
        assert R.shapes(*c["size"])[-1][:2] == (7, 7)
