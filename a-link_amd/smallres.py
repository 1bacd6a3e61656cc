"""smallres — SmallRes, the end-to-end-trained low-resolution siamese CNN (reference
code/siamese.py:134-184; driver code/ALINK_MTP.py:107,121,255).

`SmallResNet` is the Keras-Model-like object (`siamese_net`): predict / train_on_batch / test_on_batch /
fit / get_weights / set_weights / save_weights / load_weights, all on libalink_hip.so (smallres.hip).
Dropout masks are drawn on the host with np.random (the reference's come from TensorFlow's op-level
RNG, which cannot be reproduced; the distribution — keep probability 0.75, scale 1/0.75 — is the same).
"""
import contextlib
import ctypes as C

import numpy as np

from . import _abi
from .head import KerasFitMixin, glorot_uniform
from .net_host import Handle

MAXN = 256
_NO_CONTEXT = contextlib.nullcontext()


def identify_rows(scores, col=1, true_ids=None):
    """(flat_argmax, best, rank) of a (P, G, C) — or (P, G): one column — CUDA float32 score array, one row reduction per probe on
    the device (alink_identify_rows), as int32 CUDA tensors of length P; nothing synchronises.
      flat_argmax[p]: np.argmax of the row flattened to G * C — the index the reference compares with the person id
                      (code/ALINK_MTP.py:285-287);
      best[p] (EXTENSION): the lowest g maximising scores[p][g][col];
      rank[p] (EXTENSION; None without true_ids): the 0-based place of gallery true_ids[p] in a stable descending sort of
                      column col, -1 where true_ids[p] is outside 0 .. G - 1."""
    import torch
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype is torch.float32 and scores.is_contiguous()
            and scores.dim() in (2, 3)):
        raise ValueError("scores must be a contiguous (P, G, C) or (P, G) float32 CUDA tensor")
    P, G = int(scores.shape[0]), int(scores.shape[1])
    Cn = int(scores.shape[2]) if scores.dim() == 3 else 1
    dev = scores.device
    lib = _abi.init(dev.index)
    flat = torch.empty(P, dtype=torch.int32, device=dev)
    best = torch.empty(P, dtype=torch.int32, device=dev)
    rank = true = None
    if true_ids is not None:
        if isinstance(true_ids, torch.Tensor):
            true = true_ids.to(dev, torch.int32).reshape(-1).contiguous()
        else:
            true = torch.from_numpy(np.ascontiguousarray(true_ids, dtype=np.int32).reshape(-1)).to(dev)
        if true.numel() != P:
            raise ValueError("true_ids must hold one gallery index per probe (%d), got %d" % (P, true.numel()))
        rank = torch.empty(P, dtype=torch.int32, device=dev)
    _abi.check(lib.alink_identify_rows(_abi.ptr(scores), P, G, Cn, int(col), _abi.ptr(true), _abi.ptr(flat), _abi.ptr(best),
                                       _abi.ptr(rank), _abi.current_stream(dev)), "alink_identify_rows")
    return flat, best, rank


class SmallResNet(KerasFitMixin, Handle):
    prefix = "alink_smallres"

    def __init__(self, image_shape, feat, lr=1.0, rho=0.95, eps=1e-8, seed=None, device=None, prescale=False):
        device = self._open(device)                   # None: the current torch device
        torch, self.device = self.torch, "cuda:%d" % device
        self.H, self.W = int(image_shape[0]), int(image_shape[1])
        assert int(image_shape[2]) == 3
        self.feat = int(feat)
        with _abi.on_device(device):
            self.h = self.lib.alink_smallres_create(self.H, self.W, self.feat, lr, rho, eps)
        if not self.h:
            raise _abi.AlinkError("alink_smallres_create: " + self.lib.alink_last_error().decode())
        self.lr = lr
        a, b = C.c_int(), C.c_int()
        _abi.check(self.lib.alink_smallres_mask_sizes(self.h, C.byref(a), C.byref(b)))
        self.mask_sizes = (a.value, b.value)
        self.flat = b.value
        self.training_dropout = True
        rng = np.random.RandomState(seed) if seed is not None else np.random
        ws = []
        for ci, co in ((3, 32), (32, 32), (32, 64), (64, 64)):
            lim = np.sqrt(6.0 / (9 * ci + 9 * co))               # glorot_uniform on (3,3,ci,co)
            ws += [rng.uniform(-lim, lim, (3, 3, ci, co)).astype(np.float32), np.zeros(co, np.float32)]
        ws += [glorot_uniform(rng, self.flat, self.feat), np.zeros(self.feat, np.float32)]
        ws += [glorot_uniform(rng, self.feat, 128), np.zeros(128, np.float32), glorot_uniform(rng, 128, 32),
               np.zeros(32, np.float32), glorot_uniform(rng, 32, 2), np.zeros(2, np.float32)]
        self.set_weights(ws)
        self._metrics = torch.zeros(2, dtype=torch.float32, device=self.device)
        # {loss, accuracy} of a step land in pinned host memory, written by the kernel itself (as DenseHead's do): a step ends with
        # one stream wait instead of a device-to-host copy
        self._metrics_host = torch.zeros(2, dtype=torch.float32).pin_memory()
        self._metrics_np = np.zeros(2, dtype=np.float32)
        self._tdev = torch.device(self.device)
        self._tdev_index = self._tdev.index
        self._mask_buf = {}
        # Optional, OFF: train_on_batch can replay its ~40 launches as ONE captured graph (use_graph = True + alink_smallres_set_graph):
        # a stream of this model's own (torch's default stream is the NULL stream, which cannot be captured) and staging buffers that
        # keep the operands at stable addresses.  Measured on MI355X / ROCm 7.2: 0.457 ms per 16-pair step replayed against 0.375
        # as plain launches (tools/experiments/smallres_graph_ab.py) — a replayed node costs more than a launch here.
        self._stream = torch.cuda.Stream(device=self._tdev)
        self._stage = {}
        self._pin = {}
        self.use_graph = False
        self.prescale = 1 if prescale else 0

    def _shapes(self):
        return [(3, 3, 3, 32), (32,), (3, 3, 32, 32), (32,), (3, 3, 32, 64), (64,), (3, 3, 64, 64), (64,),
                (self.flat, self.feat), (self.feat,), (self.feat, 128), (128,), (128, 32), (32,), (32, 2), (2,)]

    def set_weights(self, ws):
        shapes = self._shapes()
        assert len(ws) == len(shapes)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(w, np.float32).reshape(s).ravel()
                                                    for w, s in zip(ws, shapes)]), dtype=np.float32)
        _abi.check(self.lib.alink_smallres_set_params(self.h, _abi.ptr(flat), flat.size), "alink_smallres_set_params")

    def get_weights(self):
        n = self.lib.alink_smallres_num_params(self.h)
        flat = np.empty(n, dtype=np.float32)
        _abi.check(self.lib.alink_smallres_get_params(self.h, _abi.ptr(flat), n), "alink_smallres_get_params")
        out, o = [], 0
        for s in self._shapes():
            k = int(np.prod(s))
            out.append(flat[o:o + k].reshape(s).copy())
            o += k
        return out

    def get_lr(self):
        return self.lr

    def set_lr(self, lr):
        self.lr = float(lr)
        _abi.check(self.lib.alink_smallres_set_lr(self.h, float(lr)))

    def save_weights(self, path):
        """Keras save_weights of the graph at reference code/siamese.py:139-168: the shared tower is
        one nested layer `sequential_1` holding conv2d_1..4 and dense_1; the head is dense_2..4."""
        ws = self.get_weights()
        if path.endswith(".npz"):
            np.savez(path, *ws)
            return
        from . import hdf5_lite
        tower = []
        for i, n in enumerate(["conv2d_1", "conv2d_2", "conv2d_3", "conv2d_4", "dense_1"]):
            tower += [("%s/kernel:0" % n, ws[2 * i]), ("%s/bias:0" % n, ws[2 * i + 1])]
        layers = [("input_1", []), ("input_2", []), ("sequential_1", tower), ("lambda_1", [])]
        for j, n in enumerate(["dense_2", "dense_3", "dense_4"]):
            layers.append((n, [("%s/kernel:0" % n, ws[10 + 2 * j]), ("%s/bias:0" % n, ws[11 + 2 * j])]))
        layers.append(("activation_7", []))
        hdf5_lite.save_keras_weights(path, layers)

    def load_weights(self, path):
        with open(path, "rb") as f:
            magic = f.read(4)
        if magic == b"PK\x03\x04":
            with np.load(path) as z:
                self.set_weights([z["arr_%d" % i] for i in range(len(self._shapes()))])
            return
        from . import hdf5_lite
        flat = [a for _, ws in hdf5_lite.load_keras_weights(path) for _, a in ws]
        shapes = self._shapes()
        if len(flat) != len(shapes) or any(tuple(a.shape) != tuple(s) for a, s in zip(flat, shapes)):
            raise ValueError("weight file does not match this SmallRes (%d tensors, expected %d)" % (len(flat), len(shapes)))
        self.set_weights(flat)

    def _dev(self, a):
        torch = self.torch
        if isinstance(a, torch.Tensor):
            return a.to(self.device, torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def predict(self, X, batch_size=1024, verbose=0):
        as_torch = isinstance(X[0], self.torch.Tensor)
        L, R = self._dev(X[0]), self._dev(X[1])
        n = L.shape[0]
        self._check_pairs(L, R)
        out = self.torch.empty((n, 2), dtype=self.torch.float32, device=self.device)
        for s in range(0, n, MAXN):
            m = min(MAXN, n - s)
            _abi.check(self.lib.alink_smallres_forward(self.h, _abi.ptr(L[s:s + m]), _abi.ptr(R[s:s + m]), m,
                                                       self.prescale, _abi.ptr(out[s:s + m]), _abi.current_stream(self.device)),
                       "alink_smallres_forward")
        return out if as_torch else out.cpu().numpy()

    def _check_pairs(self, L, R):
        """the kernels read n * H * W * 3 floats of the MODEL's size from each side, whatever the arrays hold (Keras raises here too)"""
        if L.shape[0] == 0 and R.shape[0] == 0:          # an empty batch reads nothing, whatever shape it arrives in
            return
        if tuple(L.shape) != (L.shape[0], self.H, self.W, 3) or tuple(R.shape) != tuple(L.shape):
            raise ValueError("expected two (n, %d, %d, 3) image batches, got %s and %s" % (self.H, self.W, tuple(L.shape), tuple(R.shape)))

    def score_pairs(self, L, R, out=None, prescale=None):
        """P(class) of the pairs (L[i], R[i]) as an (n, 2) CUDA float32 tensor (`out`, or a new one) — EXTENSION: the objective of
        the few-pixel search (attack.py's pixel scorer).  Unlike predict, row i has the same BITS whatever n, whatever chunk of
        MAXN it falls into and wherever it stands in the call (alink_smallres_score_pairs: every GEMM under a plan that is a
        function of the layer only), so an image scored among 12,800 candidates scores as it does alone.  Device tensors in and
        out, any n, enqueued on the current stream of the model's device without synchronising.  prescale (None: this model's
        own setting) = 1: raw 0..255 pixels, (x - 128) / 128 applied by the first kernel."""
        torch = self.torch
        L, R = self._dev(L), self._dev(R)
        self._check_pairs(L, R)
        n = L.shape[0]
        if out is None:
            out = torch.empty((n, 2), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (n, 2) or out.dtype is not torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous (%d, 2) float32 CUDA tensor" % n)
        pre = self.prescale if prescale is None else (1 if prescale else 0)
        _abi.check(self.lib.alink_smallres_score_pairs(self.h, _abi.ptr(L), _abi.ptr(R), n, pre, _abi.ptr(out),
                                                       _abi.current_stream(self.device)), "alink_smallres_score_pairs")
        return out

    def _out(self, out, shape):
        torch = self.torch
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != tuple(shape) or out.dtype is not torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous %s float32 CUDA tensor" % (tuple(shape),))
        return out

    def features(self, images, out=None, prescale=None):
        """The shared tower's output relu(Dense(flatten(tower(image)))) of every image, as an (n, feat) CUDA float32 tensor (`out`,
        or a new one) — EXTENSION: what the pair head takes, computed once per FACE instead of once per pair occurrence (gallery
        identification: `score_matrix`, siamese.SmallRes.identify).  Device tensors or arrays, any n, chunked inside the library
        by 512 images, enqueued on the current stream of the model's device without synchronising.  Under score_pairs' fixed
        plan (alink_smallres_features): an image has the same BITS alone, in any batch and at any position, and the bits it has
        inside score_pairs.  prescale as for score_pairs."""
        x = self._dev(images)
        n = x.shape[0]
        if n and tuple(x.shape) != (n, self.H, self.W, 3):
            raise ValueError("expected an (n, %d, %d, 3) image batch, got %s" % (self.H, self.W, tuple(x.shape)))
        out = self._out(out, (n, self.feat))
        pre = self.prescale if prescale is None else (1 if prescale else 0)
        _abi.check(self.lib.alink_smallres_features(self.h, _abi.ptr(x), n, pre, _abi.ptr(out), _abi.current_stream(self.device)),
                   "alink_smallres_features")
        return out

    def score_matrix(self, FL, FR, col=-1, out=None):
        """scores[i][j] = softmax(head(|FL[i] - FR[j]|)) of two feature matrices (`features`) through the model's own pair head —
        EXTENSION: an (nL, nR, 2) CUDA float32 tensor, or (nL, nR) holding column `col` alone (col = 0 / 1).  The pairs are
        enumerated by the kernel, nothing is materialised; element [i][j] has the bits score_pairs gives the pixel pair.  At most
        2^28 scores (nL * nR * 2) per call: walk a larger matrix in blocks of rows."""
        FL, FR = self._dev(FL), self._dev(FR)
        for F in (FL, FR):
            if F.dim() != 2 or F.shape[1] != self.feat:
                raise ValueError("expected (n, %d) feature matrices, got %s and %s" % (self.feat, tuple(FL.shape), tuple(FR.shape)))
        if col not in (-1, 0, 1):
            raise ValueError("col must be -1 (both columns), 0 or 1, got %r" % (col,))
        nL, nR = FL.shape[0], FR.shape[0]
        out = self._out(out, (nL, nR, 2) if col < 0 else (nL, nR))
        _abi.check(self.lib.alink_smallres_score_features(self.h, _abi.ptr(FL), nL, _abi.ptr(FR), nR, int(col), _abi.ptr(out),
                                                          _abi.current_stream(self.device)), "alink_smallres_score_features")
        return out

    def input_gradients(self, x, y, sample_weight=None, reduction="mean", prescale=None):
        """(dL, dR): the gradient of the Keras loss of the pairs x = [L, R] against the one-hot targets y — the inference forward,
        no Dropout — with respect to the pixels of both sides, as CUDA float32 tensors of the inputs' shape (EXTENSION: what
        noise.FGSM / PGD step along on a pixel student).  Host arrays or device tensors; any number of pairs, chunked by MAXN,
        and the result is the gradient of the WHOLE call's loss whatever the chunking: reduction="mean" is the sample-weighted
        batch mean over all rows (1 / count(sample_weight != 0)), "sum" the sum — each pair then gets the gradient of its own
        loss, whatever batch it arrives in.  prescale (None: this model's own setting) = 1: the inputs are raw 0..255 pixels, the
        first kernel applies (x - 128) / 128 and the gradient is with respect to the raw pixels.
        Parameters and optimizer state are untouched; the handle's activation buffers and the head's gradient buffer are
        overwritten, so not between dp_local_grads and dp_apply (include/alink_hip.h).
        Known limit: sgemm's split plan depends on the batch size, so the BITS of a pair's gradient can depend on the batch it
        arrives in (signs can differ where the gradient is within rounding of zero)."""
        torch = self.torch
        if reduction not in ("mean", "sum"):
            raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
        L, R, yd = self._dev(x[0]), self._dev(x[1]), self._dev(y)
        n = L.shape[0]
        if tuple(L.shape) != (n, self.H, self.W, 3) or tuple(R.shape) != tuple(L.shape) or tuple(yd.shape) != (n, 2):
            raise ValueError("expected two (n, %d, %d, 3) image batches and (n, 2) targets, got %s, %s, %s"
                             % (self.H, self.W, tuple(L.shape), tuple(R.shape), tuple(yd.shape)))
        swd = None if sample_weight is None else self._dev(sample_weight).reshape(n)
        if reduction == "sum":
            scale = 1.0
        else:
            scale = 1.0 / max(1, n if swd is None else int((swd != 0).sum()))
        pre = self.prescale if prescale is None else (1 if prescale else 0)
        dL, dR = torch.empty_like(L), torch.empty_like(R)
        st = _abi.current_stream(self.device)
        for s in range(0, n, MAXN):
            m = min(MAXN, n - s)
            _abi.check(self.lib.alink_smallres_input_grad(self.h, _abi.ptr(L[s:s + m]), _abi.ptr(R[s:s + m]), _abi.ptr(yd[s:s + m]),
                                                          _abi.ptr(None if swd is None else swd[s:s + m]), m, pre, scale,
                                                          _abi.ptr(dL[s:s + m]), _abi.ptr(dR[s:s + m]), None, st),
                       "alink_smallres_input_grad")
        return dL, dR

    def draw_masks(self, n):
        """keep-masks (u8) for the 2n tower passes: Dropout(0.25) after each pool (code/siamese.py:146,153) — on the host, for callers
        that pass `masks=` explicitly (the parity tests hand the same masks to the oracle); train_on_batch draws its own on the device."""
        e1, e2 = self.mask_sizes
        return (np.random.rand(2 * n * e1 + 2 * n * e2) >= 0.25).astype(np.uint8)

    def _staged(self, key, a, dtype=None):
        """a device tensor holding `a` at an address that is the same from step to step (host array, or device tensor on any stream
        the caller has made this model's stream wait for)"""
        torch = self.torch
        dtype = dtype or torch.float32
        if isinstance(a, torch.Tensor):
            src = a
        else:
            src = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8 if dtype is torch.uint8 else np.float32))
        buf = self._stage.get((key, tuple(src.shape)))
        if buf is None:
            buf = self._stage[(key, tuple(src.shape))] = torch.empty(tuple(src.shape), dtype=dtype, device=self.device)
        buf.copy_(src, non_blocking=True)
        return buf

    def _up(self, key, a):
        """operand `a` as a float32 device tensor: device tensors as they are, a host array through a pinned staging buffer and an
        asynchronous copy (a pageable upload is a synchronous ~15 us each); the step ends with a stream synchronisation, so the
        buffer is free again by the next one."""
        torch = self.torch
        if isinstance(a, torch.Tensor):
            if a.dtype is torch.float32 and a.is_cuda and a.is_contiguous() and a.device.index == self._tdev_index:
                return a
            return a.to(self.device, torch.float32).contiguous()
        a = np.asarray(a, dtype=np.float32)
        buf = self._pin.get((key, a.shape))
        if buf is None:
            t = torch.empty(a.shape, dtype=torch.float32).pin_memory()
            buf = self._pin[(key, a.shape)] = (t, t.numpy(), torch.empty(a.shape, dtype=torch.float32, device=self.device))
        buf[1][...] = a
        buf[2].copy_(buf[0], non_blocking=True)
        return buf[2]

    def _up_all(self, arrays):
        """the host arrays of one step (images of both sides, targets, sample weights) through ONE pinned staging buffer and ONE
        asynchronous copy into a device buffer kept from step to step (three copies and three allocations until round 6):
        returns the device views, or None if any operand is not a host array (those go through _up one by one)."""
        torch = self.torch
        if any(isinstance(a, torch.Tensor) for a in arrays if a is not None):
            return None
        arrs = [None if a is None else np.asarray(a, dtype=np.float32) for a in arrays]
        key = tuple(None if a is None else a.shape for a in arrs)
        ent = self._pin.get(key)
        if ent is None:
            offs, o = [], 0
            for a in arrs:
                offs.append(o)
                o += 0 if a is None else (a.size + 63) // 64 * 64          # 256-byte aligned pieces
            host = torch.empty(max(o, 64), dtype=torch.float32).pin_memory()
            dev = torch.empty(max(o, 64), dtype=torch.float32, device=self.device)
            hv = host.numpy()
            views = [None if a is None else hv[f:f + a.size].reshape(a.shape) for a, f in zip(arrs, offs)]
            dviews = [None if a is None else dev[f:f + a.size].view(a.shape) for a, f in zip(arrs, offs)]
            ent = self._pin[key] = (host, dev, views, dviews, o)
        host, dev, views, dviews, o = ent
        for v, a in zip(views, arrs):
            if a is not None:
                v[...] = a
        dev.copy_(host, non_blocking=True)
        return dviews

    def train_on_batch(self, x, y, class_weight=None, sample_weight=None, masks=None):
        torch = self.torch
        n = len(y)
        assert n <= MAXN, "train batches larger than %d pairs are not supported" % MAXN
        sw = sample_weight
        if sw is None and class_weight is not None:
            sw = np.asarray([class_weight[c] for c in np.asarray(y).argmax(axis=1)], np.float32)
        cur = torch.cuda.current_stream(self._tdev)
        if masks is None and not self.use_graph and not isinstance(x[0], torch.Tensor) and not isinstance(x[1], torch.Tensor) \
                and not isinstance(y, torch.Tensor) and not isinstance(sw, torch.Tensor):
            # host operands, as the reference's Keras call hands them: ONE synchronous library call stages them (pinned memory of the
            # handle, one upload), draws the masks, runs the step, synchronises and returns {loss, accuracy}
            L, R = np.ascontiguousarray(x[0], np.float32), np.ascontiguousarray(x[1], np.float32)
            yh = np.ascontiguousarray(y, np.float32)
            swh = None if sw is None else np.ascontiguousarray(sw, np.float32)
            drop = 1 if self.training_dropout else 0
            seed = int(np.random.randint(0, 2 ** 31 - 1)) if drop else 0      # (one np.random draw per step, as in the device-operand form)
            _abi.check(self.lib.alink_smallres_train_on_batch_host(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yh), _abi.ptr(swh), n, self.prescale,
                                                                   drop, seed, _abi.ptr(self._metrics_np), C.c_void_p(cur.cuda_stream)),
                       "alink_smallres_train_on_batch_host")
            return self._metrics_np.tolist()
        st = self._stream if self.use_graph else cur
        if st is not cur:
            st.wait_stream(cur)                       # inputs produced on the caller's stream
        # (entering a stream context costs ~5 us of host time before the step's first launch, with the device idle: only when
        # the step runs on another stream than the caller's)
        with (torch.cuda.stream(st) if st is not cur else _NO_CONTEXT):
            if self.use_graph:
                L, R, yd = self._staged("L", x[0]), self._staged("R", x[1]), self._staged("y", y)
                swd = self._staged("sw", sw) if sw is not None else None
            else:
                staged = self._up_all((x[0], x[1], y, sw))
                if staged is not None:
                    L, R, yd, swd = staged
                else:
                    L, R, yd = self._up("L", x[0]), self._up("R", x[1]), self._up("y", y)
                    swd = self._up("sw", sw) if sw is not None else None
            if masks is None and self.training_dropout:
                # the keep-masks are drawn ON THE DEVICE (Philox, keyed by one 31-bit seed taken from np.random per step): drawing
                # 2n(e1 + e2) = 304,128 uniforms with np.random on the host was 0.74 of the step's 1.68 ms.  One np.random draw per step
                # keeps the ranks of a multi-rank loop in step (alink_loop.sync_host_randomness) like the host-drawn masks did.
                # They are drawn by the step's own first launch (alink_smallres_train_step_drawn: the bytes alink_keep_masks writes).
                e1, e2 = self.mask_sizes
                md = self._mask_buf.get(n)               # (a step's masks are consumed by that step, in stream order)
                if md is None:
                    md = self._mask_buf[n] = torch.empty(2 * n * (e1 + e2), dtype=torch.uint8, device=self.device)
                _abi.check(self.lib.alink_smallres_train_step_drawn(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), _abi.ptr(swd), n,
                                                                    self.prescale, _abi.ptr(md), int(np.random.randint(0, 2 ** 31 - 1)), 0.0, 1,
                                                                    C.c_void_p(self._metrics_host.data_ptr()), C.c_void_p(st.cuda_stream)),
                           "alink_smallres_train_step_drawn")
            else:
                if masks is not None:
                    md = self._staged("masks", masks, torch.uint8) if self.use_graph else \
                        torch.from_numpy(np.ascontiguousarray(masks, np.uint8)).to(self.device)
                else:
                    md = None
                _abi.check(self.lib.alink_smallres_train_step(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), _abi.ptr(swd), n,
                                                              self.prescale, _abi.ptr(md), 0.0, 1, C.c_void_p(self._metrics_host.data_ptr()),
                                                              C.c_void_p(st.cuda_stream)), "alink_smallres_train_step")
        st.synchronize()
        return self._metrics_host.tolist()

    # -- data-parallel step (distributed.dp_train_on_batch) --------------------------------------------
    # Rows from which the step is SHARDED in mode "auto".  One 16-pair step is 0.35 ms on one MI355X (profiles/r06d_*); its flat
    # gradient buffer is 20.2 MB at 32 x 32 / 2048 — an 8-rank exchange moves 7 x 20 MB into every rank over 7 xGMI links
    # (~150 GB/s each: >= 0.15 ms before any latency) plus the sum.  Replicas fed the same batch and the same mask seed stay
    # bit-identical, so below ~8 steps' worth of rows per rank replication wins; the threshold is that estimate — no multi-GPU
    # node was available to measure it — and `mode="sharded"` forces the exchange at any size.
    DP_SHARD_MIN_ROWS = 128

    def grads_tensor(self, with_metrics=False):
        """torch alias of the flat [tower | head] gradient buffer (for torch.distributed collectives); with_metrics appends
        the 4 spare floats that follow it (slot 0 / 1: loss, accuracy of a data-parallel step)."""
        torch = self.torch
        n = self.lib.alink_smallres_num_params(self.h) + (4 if with_metrics else 0)

        class _CAI(object):
            pass
        holder = _CAI()
        holder.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (int(self.lib.alink_smallres_grads_dev(self.h)), False),
                                           "version": 2, "strides": None}
        t = torch.as_tensor(holder, device=self.device)
        t._alink_owner = self
        return t

    def dp_begin(self, n, group):
        """the step's dropout seed: every rank draws one (np.random stays in step on all ranks, as in the replicated form)
        and rank 0's is the one used"""
        seed = int(np.random.randint(0, 2 ** 31 - 1)) if self.training_dropout else -1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            box = [seed]
            dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
            seed = int(box[0])
        return seed

    def _masks_of_rows(self, lo, hi, n, seed):
        """the keep-masks the whole-batch step (train_on_batch: one stream of 2n(e1 + e2) elements, [L ; R] image order per
        pool) draws for pair rows lo : hi, in the layout of a batch of hi - lo pairs"""
        e1, e2 = self.mask_sizes
        k = hi - lo
        md = self.torch.empty(2 * k * (e1 + e2), dtype=self.torch.uint8, device=self.device)
        st = _abi.current_stream(self.device)
        parts = ((0, lo * e1, k * e1), (k * e1, (n + lo) * e1, k * e1),                       # pool 1: L rows, R rows
                 (2 * k * e1, 2 * n * e1 + lo * e2, k * e2), (2 * k * e1 + k * e2, 2 * n * e1 + (n + lo) * e2, k * e2))
        for dst, first, count in parts:
            _abi.check(self.lib.alink_keep_masks_at(_abi.ptr(md[dst:dst + count]), count, 0.75, seed, first, st), "alink_keep_masks_at")
        return md

    def dp_local_grads(self, x, y, w_all, lo, hi, n, grad_scale, m, ctx):
        take = lambda a: a[lo:hi] if hasattr(a, "shape") else np.asarray(a)[lo:hi]
        L, R, yd = self._dev(take(x[0])), self._dev(take(x[1])), self._dev(take(y))
        swd = None if w_all is None else self._dev(w_all[lo:hi])
        k = hi - lo
        assert k <= MAXN, "a rank's slice of more than %d pairs is not supported" % MAXN
        md = self._masks_of_rows(lo, hi, n, ctx) if (self.training_dropout and ctx is not None and ctx >= 0) else None
        _abi.check(self.lib.alink_smallres_train_step(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), _abi.ptr(swd), k,
                                                      self.prescale, _abi.ptr(md), grad_scale, 0, _abi.ptr(m),
                                                      _abi.current_stream(self.device)), "alink_smallres_train_step")

    def dp_apply(self):
        _abi.check(self.lib.alink_smallres_apply_update(self.h, _abi.current_stream(self.device)), "alink_smallres_apply_update")

    def test_on_batch(self, x, y):
        n = len(y)
        if n <= MAXN:
            # one evaluation launch chain: operands through the step's staging (one upload), {loss, accuracy} written by the
            # device into pinned host memory, one stream synchronisation (a .to() per operand and a .cpu() of the metrics were a
            # third of the call)
            torch = self.torch
            staged = self._up_all((x[0], x[1], y, None))
            if staged is not None:
                L, R, yd, _ = staged
            else:
                L, R, yd = self._up("L", x[0]), self._up("R", x[1]), self._up("y", y)
            st = torch.cuda.current_stream(self._tdev)
            _abi.check(self.lib.alink_smallres_eval(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), n, self.prescale,
                                                    C.c_void_p(self._metrics_host.data_ptr()), C.c_void_p(st.cuda_stream)), "alink_smallres_eval")
            st.synchronize()
            return self._metrics_host.tolist()[:2]
        L, R, yd = self._dev(x[0]), self._dev(x[1]), self._dev(y)
        tot, seen = np.zeros(2), 0
        for s in range(0, L.shape[0], MAXN):
            m = min(MAXN, L.shape[0] - s)
            _abi.check(self.lib.alink_smallres_eval(self.h, _abi.ptr(L[s:s + m]), _abi.ptr(R[s:s + m]),
                                                    _abi.ptr(yd[s:s + m]), m, self.prescale, _abi.ptr(self._metrics),
                                                    _abi.current_stream(self.device)), "alink_smallres_eval")
            tot += self._metrics.cpu().numpy() * m
            seen += m
        return [float(tot[0] / seen), float(tot[1] / seen)]
