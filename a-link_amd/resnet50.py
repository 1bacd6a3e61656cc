"""VGGResNet50 — host-side owner of one alink_resnet50_t handle: the keras-vggface ResNet-50 the
reference builds at code/siamese.py:203-209, with the slice of the Keras Model API it uses (`predict`).

Weights: a Keras weight file (the `rcmalli_vggface_tf_notop_resnet50.h5` keras-vggface downloads; read
with hdf5_lite.py), a dict of arrays with Keras names, or synthetic (He-normal convs, BN statistics
as in weights.synthetic_ir_params) when nothing is given — there is no network here to fetch the
pretrained file.
"""
import ctypes as C

import numpy as np

from . import _abi
from .net_host import ImageNet

UNITS = (3, 4, 6, 3)
MID = (64, 128, 256, 512)
MEAN_BGR = (91.4953, 103.8827, 131.0912)


def tensor_shapes():
    """Ordered {name: shape}: "<layer>/kernel" (kh, kw, in, out) and "<layer>/bn/<stat>" (out,)."""
    t = {}

    def conv(name, k, cin, cout):
        t[name + "/kernel"] = (k, k, cin, cout)
        for s in ("gamma", "beta", "moving_mean", "moving_variance"):
            t[name + "/bn/" + s] = (cout,)
    conv("conv1/7x7_s2", 7, 3, 64)
    cin = 64
    for s in range(4):
        mid, out = MID[s], 4 * MID[s]
        for u in range(1, UNITS[s] + 1):
            p = "conv%d_%d_" % (s + 2, u)
            conv(p + "1x1_reduce", 1, cin, mid)
            conv(p + "3x3", 3, mid, mid)
            conv(p + "1x1_increase", 1, mid, out)
            if u == 1:
                conv(p + "1x1_proj", 1, cin, out)
            cin = out
    return t


def synthetic_params(seed=1):
    rng = np.random.default_rng(seed)
    p = {}
    for name, shape in tensor_shapes().items():
        if name.endswith("/kernel"):
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[0] * shape[1] * shape[2]))
        elif name.endswith("gamma"):
            # the last BN of a unit small, as trained residual nets have it: keeps activations bounded over 16 units
            v = rng.uniform(0.2, 0.5, shape) if "increase" in name else rng.uniform(0.5, 1.5, shape)
        elif name.endswith("beta") or name.endswith("moving_mean"):
            v = rng.standard_normal(shape) * 0.1
        else:
            v = rng.uniform(0.5, 1.5, shape)
        p[name] = np.ascontiguousarray(v, dtype=np.float32)
    return p


def load_keras_h5(path):
    """Keras weight file -> {"<layer>/kernel": ..., "<layer>/bn/gamma": ...} (the C library's names)."""
    from . import hdf5_lite
    out = {}
    for lname, ws in hdf5_lite.load_keras_weights(path):
        for wname, arr in ws:
            leaf = wname.rsplit("/", 1)[-1].split(":")[0]      # kernel | gamma | beta | moving_mean | moving_variance
            out[lname + "/" + leaf] = np.ascontiguousarray(arr, dtype=np.float32)
    return out


def save_keras_h5(path, params):
    from . import hdf5_lite
    layers = []
    for name in tensor_shapes():
        if name.endswith("/kernel"):
            l = name[:-len("/kernel")]
            layers.append((l, [(l + "/kernel:0", params[name])]))
            layers.append((l + "/bn", [(l + "/bn/%s:0" % s, params[l + "/bn/" + s])
                                       for s in ("gamma", "beta", "moving_mean", "moving_variance")]))
    hdf5_lite.save_keras_weights(path, layers)


class VGGResNet50(ImageNet):
    prefix = "alink_resnet50"
    DTYPES = {"bf16": _abi.DT_BF16, "f16": _abi.DT_F16, "f16x2": _abi.DT_F16X2}

    def __init__(self, image_size=(224, 224), weights=None, dtype="bf16", device=None, max_batch=128, bn_eps=1e-3,
                 seed=1, enable_grad=False):
        self.device = self._open(device)              # None: the current torch device
        self._embed = self.lib.alink_resnet50_embed
        self.image_size = tuple(image_size)
        self.max_batch = int(max_batch)
        if weights is None:
            params = synthetic_params(seed)
        elif isinstance(weights, str):
            params = load_keras_h5(weights)
        else:
            params = weights
        # dtype "f16x2": split precision (f16 pairs, three products on the f16 matrix cores, calibrated power-of-two scales:
        # a-link_amd/backbone.py) — features to float32 accuracy, what selection through this feature model needs
        self.dtype = dtype
        # enable_grad: the input-gradient pass (FGSM / PGD extension; 16-bit modes only): embed_with_cache / input_gradient
        self.grad_enabled = bool(enable_grad)
        self._create(self.device, int(image_size[0]), int(image_size[1]), self.DTYPES[dtype], float(bn_eps))
        if enable_grad:
            _abi.check(self.lib.alink_resnet50_enable_grad(self.h), "alink_resnet50_enable_grad")
        self.load_tensors(params, "weights are")
        if dtype == "f16x2":         # scales from the three probe images; a batch that leaves the range later is
            self.calibrate(self.probe_images())      # re-calibrated on (scales only go down) and re-run

    def calibrate(self, x, preprocessed=False, merge=False):
        """dtype 'f16x2': choose the per-tensor power-of-two scales from these images (all of them, max_batch at a time;
        every chunk after the first only lowers a scale, like merge=True)."""
        if isinstance(x, np.ndarray):
            x = self.torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        pre, fn = 1 if preprocessed else 0, self.lib.alink_resnet50_calibrate
        self._calibrate_chunks(x, merge, lambda xc, n, ws, wsb, m, st: fn(self.h, _abi.ptr(xc), n, pre, ws, wsb, m, st),
                               self.torch.float32)

    def _identity(self):
        return {"image_size": [int(v) for v in self.image_size]}

    def embed_device(self, x, preprocessed=False, out=None, _retry=True):
        """x: CUDA (N, H, W, 3) float32 — raw RGB 0..255, or preprocess()'d when preprocessed=True."""
        torch = self.torch
        self._check_input(x)
        x = x.to(torch.float32).contiguous()
        n = x.shape[0]
        if out is None:
            out = torch.empty((n, 2048), dtype=torch.float32, device=x.device)
        pre, st = 1 if preprocessed else 0, _abi.current_stream(self.device)
        for i in range(0, n, self.max_batch):
            m = min(self.max_batch, n - i)
            ws, wsb = self.ws.get(m)
            _abi.check(self._embed(self.h, _abi.ptr(x[i:i + m]), m, pre, _abi.ptr(out[i:i + m]), ws, wsb, st), "alink_resnet50_embed")
        return self._checked(out, x if _retry else None, (preprocessed,))   # never hand back non-finite features silently

    # -- input gradient (FGSM / PGD extension) --------------------------------------------------------
    def embed_with_cache(self, x, preprocessed=False):
        """Forward on <= max_batch images keeping what input_gradient needs: embed_device's features, bit for bit.
        x: CUDA (n, H, W, 3) float32, raw RGB or (preprocessed=True) preprocess()'d."""
        _, x, n, out, ws, wsb = self._cache_args(x, 2048)
        pre = 1 if preprocessed else 0
        _abi.check(self.lib.alink_resnet50_embed_cached(self.h, _abi.ptr(x), n, pre, _abi.ptr(out), ws, wsb,
                                                        _abi.current_stream(self.device)), "alink_resnet50_embed_cached")
        self._cached = (n, pre)
        return self._checked(out)                     # f16 raises (the gradient pass has no f16x2 form to re-calibrate)

    def input_gradient(self, dfeat):
        """d(loss)/d(pixels) for the batch of the last embed_with_cache, given dfeat = d(loss)/d(feature), (n, 2048) float32
        CUDA.  (n, H, W, 3) float32 in the channel order of that forward's input (raw RGB unless it was preprocessed)."""
        (n, pre), dfeat, ws, wsb = self._grad_args(dfeat, 2048)
        dpix = self.torch.empty((n,) + self.image_size + (3,), dtype=self.torch.float32, device=dfeat.device)
        _abi.check(self.lib.alink_resnet50_input_grad(self.h, _abi.ptr(dfeat), n, pre, _abi.ptr(dpix), ws, wsb,
                                                      _abi.current_stream(self.device)), "alink_resnet50_input_grad")
        return dpix

    def predict(self, X, batch_size=128, verbose=0, preprocessed=True):
        """Keras Model.predict on PREPROCESSED input (what RESNET50.process passes, code/siamese.py:216)."""
        torch = self.torch
        if isinstance(X, torch.Tensor):
            return self.embed_device(X.to("cuda:%d" % self.device), preprocessed)
        X = np.ascontiguousarray(np.asarray(X), dtype=np.float32)
        if len(X) == 0:
            return np.zeros((0, 2048), np.float32)
        return self.embed_device(torch.from_numpy(X).to("cuda:%d" % self.device), preprocessed).cpu().numpy()

    def profile(self, x):
        """One profiled forward on raw pixels: list of (op name, ms, flops)."""
        n = x.shape[0]
        out = self.torch.empty((n, 2048), dtype=self.torch.float32, device=x.device)
        ws, wsb = self.ws.get(n)
        cap = 128
        ms, fl, k = (C.c_float * cap)(), (C.c_double * cap)(), C.c_int(cap)
        _abi.check(self.lib.alink_resnet50_profile(self.h, _abi.ptr(x), n, _abi.ptr(out), ws, wsb,
                                                   _abi.current_stream(self.device), ms, fl, C.byref(k)), "alink_resnet50_profile")
        return [(self.lib.alink_resnet50_op_name(self.h, i).decode(), ms[i], fl[i]) for i in range(k.value)]
