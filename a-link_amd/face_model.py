"""face_model — drop-in for reference code/face_model.py (hot path only).

    get_model(ctx, image_size, model_str, layer)   code/face_model.py:28-41
    FaceModel(args)                                code/face_model.py:43-57
    FaceModel.get_input(face_img, bbox, landmark)  code/face_model.py:70-84  (alignment when a box / landmarks are given, HWC -> CHW)
    FaceModel.get_feature(aligned)                 code/face_model.py:86-93  (forward + L2 normalise)

Differences, all deliberate: the executor is batched (`get_features`), the checkpoint is the MXNet
pair `<prefix>-symbol.json` + `<prefix>-%04d.params` read without MXNet (mxnet_format.py), an .npz
with the same tensor names, or `synthetic:<arch>`, and the MTCNN detector / gender-age model that the
reference constructs but never uses (code/face_model.py:52-67,95-107) are not built.
"""
import numpy as np

from . import weights as W
from .backbone import IRBackbone


def default_dtype(enable_grad=False, small_batch_split=False):
    """The storage / arithmetic mode a model built through the reference's API gets when the caller names none:
    "f16x2" — split precision, whose active-learning selection sets equal the f32 arithmetic's (the reference computes
    in float32: code/face_model.py:90) at ~16 k IR-100 embeddings/s.  The input-gradient pass exists for 16-bit
    storage only: asking for it selects "bf16".  dtype="bf16" (44 k embeddings/s, 1 - cos ~3e-4: good for SCREENING, a
    third of a tight top-k turns over) and "f16" / "f32" remain explicit choices.  small_batch_split (the opt-in latency
    mode for batches <= 32) works in every 16-bit mode and does not change the dtype."""
    return "bf16" if enable_grad else "f16x2"


def get_model(ctx, image_size, model_str, layer, dtype=None, max_batch=292, enable_grad=False,
              small_batch_split=False):
    assert layer == "fc1", "the reference slices the symbol at fc1_output (code/face_model.py:36,53)"
    if dtype is None:
        dtype = default_dtype(enable_grad, small_batch_split)
    params, cfg = W.resolve_model_config(model_str, image_size)
    # ctx: a device index as the reference passes (mx.gpu(args.gpu), code/face_model.py:46,57); None = the process's
    # current device (one process per GPU: torch.cuda.set_device(LOCAL_RANK))
    device = int(ctx) if isinstance(ctx, (int, np.integer)) and not isinstance(ctx, bool) else None
    return IRBackbone(params, image_size=image_size, emb=cfg["emb"], dtype=dtype, device=device, max_batch=max_batch,
                      widths=cfg["widths"], bn_eps=cfg["bn_eps"], enable_grad=enable_grad,
                      small_batch_split=small_batch_split)


class FaceModel(object):
    def __init__(self, args):
        self.args = args
        _vec = args.image_size.split(',')
        assert len(_vec) == 2
        image_size = (int(_vec[0]), int(_vec[1]))
        self.model = None
        self.ga_model = None
        if len(args.model) > 0:
            self.model = get_model(getattr(args, "gpu", None), image_size, args.model, 'fc1',
                                   dtype=getattr(args, "dtype", None),
                                   max_batch=getattr(args, "max_batch", 292),
                                   enable_grad=bool(args.get("enable_grad", False)) if hasattr(args, "get") else False,
                                   small_batch_split=bool(args.get("small_batch_split", False)) if hasattr(args, "get") else False)
        self.threshold = args.threshold
        self.det_minsize = 50
        self.det_threshold = [0.6, 0.7, 0.8]
        self.image_size = image_size

    def get_input(self, face_img, bbox=None, landmark=None):
        """HWC -> CHW.  With a face box or five landmarks (from the caller's detector: none is built here) the photo is first
        cropped / aligned to 112 x 112 by face_preprocess.preprocess — the call the reference wrote and commented out
        (code/face_model.py:81), its DFW crops being cut beforehand."""
        if bbox is not None or landmark is not None:
            from . import face_preprocess
            face_img = face_preprocess.preprocess(face_img, bbox, landmark, image_size='112,112')
        return np.transpose(face_img, (2, 0, 1))

    def get_feature(self, aligned):
        """(3,H,W) float RGB 0..255 -> (emb,) float32, unit L2 norm."""
        blob = np.expand_dims(np.asarray(aligned, dtype=np.float32), axis=0)
        return self.model.embed(blob).flatten()

    def get_features(self, images):
        """Batched extension: (N,H,W,3) or (N,3,H,W) -> (N, emb).  Same arithmetic per image."""
        return self.model.embed(images)
