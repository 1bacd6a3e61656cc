"""CPU: the one-op references of tests/vgg16_ref.py are the network, their tolerance holds for a float32 device, and it catches
every mutant.

Three things, none of which needs a GPU:
  * chained without rounding, the op references reproduce oracle/vgg16.forward (and .process on raw pixels: the flip and the
    means) to float32 accuracy;
  * a stand-in device — torch's float32 convolution of the same 16-bit operands, stored in the type, fed layer by layer with
    its own outputs as the GPU test feeds the device's — stays within the tolerance at every layer.  Measured at 74 x 100, two
    images, with these draws: max err / tol 0.90 (bf16), 0.32 (f16): half an ulp of the stored value plus float32 summation;
  * every mutant of the reference leaves the tolerance in more than 1 % of the outputs of every image at every layer it
    applies to.  Measured: >= 0.43 for all but the border mutant, whose 0.02 .. 0.34 is about half the border ring's share of
    the map (the other half is outputs the ReLU zeroes either way).
"""
import numpy as np
import pytest
import torch

import vgg16_ref as R

H, W, N = 74, 100, 2
SHARE = 0.01


@pytest.fixture(scope="module")
def params():
    return R.draw_params(11)


@pytest.fixture(scope="module")
def images():
    return np.random.default_rng(5).standard_normal((N, H, W, 3)).astype(np.float32)


def _chain_unrounded(params, x, preprocessed):
    A = R.stem_pixels(x, None, preprocessed)
    for i in range(len(R.OPS)):
        A, _ = R.op_ref(params, None, i, A)
    return R.nhwc(A).reshape(A.shape[0], -1).numpy()


def test_chained_references_are_the_oracle(params, images):
    from oracle import vgg16 as O
    got, want = _chain_unrounded(params, images, True), O.forward(params, images).astype(np.float64)
    assert got.shape == want.shape == (N, (H >> 5) * (W >> 5) * 512)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    raw = np.random.default_rng(6).integers(0, 256, (1, 40, 36, 3)).astype(np.float32)
    got, want = _chain_unrounded(params, raw, False), O.process(params, raw).astype(np.float64)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()


def _beyond(mut, ref, tol):
    """per image: the share of outputs where the mutant leaves the tolerance around the reference"""
    return ((mut - ref).abs() > tol).double().mean(dim=(1, 2, 3))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_standin_within_tolerance_and_mutants_beyond(params, images, dt):
    A = R.stem_pixels(images, dt, True)
    worst, odd_pools = 0.0, 0
    for i, (kind, name) in enumerate(R.OPS):
        ref, Wt = R.op_ref(params, dt, i, A)
        if kind == "pool":
            got = ref                                        # a maximum of 16-bit values is one of them: nothing to round
            if A.shape[2] % 2 or A.shape[3] % 2:
                odd_pools += 1
                share = (R.pool_shifted(A) != ref).double().mean(dim=(1, 2, 3))
                print("%s %s %dx%d shifted window: share %s" % (dt, name, A.shape[2], A.shape[3], share.tolist()))
                assert (share > SHARE).all(), (name, share)
        else:
            b = R.bias_of(params, name)
            tol = R.tolerance(ref, A, Wt, dt)
            got = R.conv_standin(A, Wt, b, dt)
            w = R.worst(got, ref, tol)
            worst = max(worst, w)
            print("%s %s %dx%d s=%s stand-in err/tol %.3f" % (dt, name, A.shape[2], A.shape[3],
                                                               ["%.2f" % v for v in R.scale(A, Wt).flatten().tolist()], w))
            assert w <= 1.0, (name, w)
            for what, mutant in R.CONV_MUTANTS.items():
                share = _beyond(mutant(A, Wt, b), ref, tol)
                print("    %-34s share %s" % (what, ["%.3f" % v for v in share.tolist()]))
                assert (share > SHARE).all(), (name, what, share)
        A = got
    assert odd_pools == 3
    print("%s: largest stand-in err / tol %.3f" % (dt, worst))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_stem_mutants_on_raw_pixels(params, dt):
    x = np.random.default_rng(7).integers(0, 256, (N, H, W, 3)).astype(np.float32)
    Wt, b = R.weights_t(params, "conv1_1", dt), R.bias_of(params, "conv1_1")
    A = R.stem_pixels(x, dt, False)
    ref = R.conv_ref(A, Wt, b)
    tol = R.tolerance(ref, A, Wt, dt)
    assert R.worst(R.conv_standin(A, Wt, b, dt), ref, tol) <= 1.0
    # the flip and the means are the reference's own preprocessing, exactly (bf16 / f16 round the same float32 value)
    from oracle import vgg16 as O
    assert torch.equal(A, R.nchw(R.round_to(torch.from_numpy(O.preprocess_input_v1(x)), dt)))
    for what, kw in (("no flip", dict(flip=False)), ("means in RGB order", dict(means_bgr=False))):
        share = _beyond(R.conv_ref(R.stem_pixels(x, dt, False, **kw), Wt, b), ref, tol)
        print("%s stem, %s: share %s" % (dt, what, share.tolist()))
        assert (share > SHARE).all(), (what, share)
    # the product's own 0.05 biases on raw pixels: the bias mutant would go unseen (why draw_params draws 0.5).  Measured
    # share: 1.2e-4 (bf16) / 3.9e-4 (f16) of the outputs, far below what counts as seen
    from a_link_amd import vgg16 as V
    p0 = V.synthetic_params(11)
    W0, b0 = R.weights_t(p0, "conv1_1", dt), R.bias_of(p0, "conv1_1")
    ref0 = R.conv_ref(A, W0, b0)
    share = _beyond(R.conv_ref(A, W0, b0.roll(1)), ref0, R.tolerance(ref0, A, W0, dt))
    print("%s stem, 0.05 biases rolled: share %s" % (dt, share.tolist()))
    assert (share < SHARE).all(), share
