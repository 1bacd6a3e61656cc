"""ALINK_MTP — the reference's Multi-PIE low-resolution driver (code/ALINK_MTP.py) as a runnable module:

    python -m a_link_amd.ALINK_MTP --dataDirPrefix ../MultiPieSplits/split1/train --testDir ../MultiPieSplits/split1/test

Teacher: VGGFace2 ResNet-50 features at 224 x 224 scored by the ensemble; student: SmallRes trained end
to end on lowRes x lowRes pixels.  Same flags and phases: train the low-res model and quit if it is not
saved yet (code/ALINK_MTP.py:116-125), otherwise run the framework loop (alink_loop.run_alink_mtp),
save, and report top-1 identification on the test split (:271-289).
--noise adversarial (the default, code/ALINK_MTP.py:53) is the reference's few-pixel differential-evolution attack on the student:
the pairs are searched at the resolution the driver hands them and every candidate reaches the student at lowRes x lowRes through
one fused perturb + split + resize launch (attack.py's pixel scorer; all the searches of a batch in lock-step).  Its settings —
--attack_pixels 40, --attack_maxiter 50, --attack_popsize 250, the reference's (code/attack.py:91) — are options of this driver.
--noise also takes the gradient extensions `fgsm` / `pgd`: with feature_model=None they attack the student on the pixels the
driver perturbs (noise.FGSM's pixel-model route: SmallRes.input_gradients, pulled back through the resize to lowRes).
--gallery_eval (an extension, off by default) computes the closing top-1 identification with every test face embedded once
(SmallRes.identify) instead of once per (probe, gallery) pair, and adds the rank-1 / CMC figures on P(same).
"""
import argparse
import sys

from . import alink_loop, committee, noise, readDFW, readMTP, siamese

IMAGE_RES, FEATURE_RES = (224, 224), (2048,)


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    alink_loop.add_flags(p)
    p.set_defaults(out_model='MTP_models/postALINK', ensemble_basepath='MTP_models/ensemble', noise='adversarial',
                   batch_send=32, mixture_ratio=1, alink_bs=8, eps=0.1)          # code/ALINK_MTP.py:49-69
    p.add_argument("--dataDirPrefix", default="../MultiPieSplits/split1/train")
    p.add_argument("--testDir", default="../MultiPieSplits/split1/test")
    p.add_argument("--lowres_basemodel", default="MTP_models/lowresModel")
    p.add_argument("--lowRes", type=int, default=48)
    p.add_argument("--lowres_epochs", type=int, default=10)
    p.add_argument("--highres_epochs", type=int, default=5)
    p.add_argument("--resnet50_weights", default=None)
    p.add_argument("--pretrain_steps", type=int, default=32000)
    p.add_argument("--quiet", action="store_true")
    # the few-pixel search of `--noise adversarial` (PixelAttacker.attack_all's defaults, code/attack.py:91)
    p.add_argument("--attack_pixels", type=int, default=40)
    p.add_argument("--attack_maxiter", type=int, default=50)
    p.add_argument("--attack_popsize", type=int, default=250)
    # EXTENSION, off: the closing top-1 identification with every test face embedded once (alink_loop.top1_identification_gallery)
    p.add_argument("--gallery_eval", action="store_true", default=False)
    return p


def make_noise(name, model, FLAGS):
    """the noise object of one --noise entry over the student; `adversarial` takes the search settings of the command line"""
    cls = noise.get_relevant_noise(name)
    if cls is noise.AdversarialNoise:
        return cls(model=model, sess=None, feature_model=None, pixel_count=FLAGS.attack_pixels, maxiter=FLAGS.attack_maxiter,
                   popsize=FLAGS.attack_popsize)
    return cls(model=model, sess=None, feature_model=None)


def main(argv=None):
    FLAGS = build_parser().parse_args(argv)
    verbose = 0 if FLAGS.quiet else 1
    low_res = (FLAGS.lowRes, FLAGS.lowRes)
    print("== Low resolution : %s ==" % str(low_res))
    conversionModel = siamese.RESNET50(IMAGE_RES, weights=FLAGS.resnet50_weights)
    X_dig_raw = readMTP.readAllImages(FLAGS.dataDirPrefix)
    assert 0 <= FLAGS.split_ratio <= 1 and 0 <= FLAGS.disparity_ratio <= 1 and 0 <= FLAGS.eps < 0.5
    print("== Noise that will be used for ALINK: %s ==" % (FLAGS.noise))
    if FLAGS.split_ratio > 0:
        (X_dig_pre, X_dig_post) = readDFW.splitDisguiseData(X_dig_raw, pre_ratio=FLAGS.split_ratio)
    else:
        X_dig_pre = X_dig_post = X_dig_raw
    ensemble = [siamese.SiameseNetwork(FEATURE_RES, FLAGS.ensemble_basepath + str(i), 1e-1)
                for i in range(1, FLAGS.num_ensemble_models + 1)]
    lowResModel = siamese.SmallRes(low_res + (3,), FEATURE_RES, FLAGS.lowres_basemodel + str(FLAGS.lowRes), 1e-1)
    ensembleNoise = [make_noise(x, lowResModel, FLAGS) for x in FLAGS.noise.split(',')]
    bag = committee.Bagging(ensemble, ensembleNoise)
    if not lowResModel.maybeLoadFromMemory():
        print('== Training lowres-faces model ==')
        normGen = readDFW.getNormalGenerator(X_dig_pre, FLAGS.batch_size)
        lowResSiamGen = readMTP.getGenerator(normGen, FLAGS.batch_size, low_res)
        lowResModel.customTrainModel(lowResSiamGen, FLAGS.lowres_epochs, FLAGS.batch_size, 0.2, FLAGS.pretrain_steps,
                                     preprocess=True, verbose=verbose)
        lowResModel.save()
        return None
    print('== Loaded lowres-faces model from memory ==')
    for m in ensemble:
        m.maybeLoadFromMemory()
    normGen = readDFW.getNormalGenerator(X_dig_pre, FLAGS.batch_size)
    dataGen = readMTP.getGenerator(normGen, FLAGS.batch_size, low_res)
    state = alink_loop.run_alink_mtp(FLAGS, conversionModel, bag, ensembleNoise, lowResModel, X_dig_post, dataGen,
                                     IMAGE_RES, low_res, verbose=verbose)
    X_test = readMTP.readAllImages(FLAGS.testDir, low_res)
    if FLAGS.gallery_eval:
        det = {}
        state.top1 = alink_loop.top1_identification_gallery(lowResModel, X_test, details=det)
        state.identification = alink_loop.identification_stats(det["best"], det["rank"], det["true_ids"])
    else:
        state.top1 = alink_loop.top1_identification(lowResModel, X_test)
    print('Top-1 accuracy : ', state.top1)
    if FLAGS.gallery_eval:
        print('Rank-1 on P(same) (extension) : ', state.identification["rank1"], ' CMC : ', state.identification["cmc"])
    return state


if __name__ == "__main__":
    main(sys.argv[1:])
