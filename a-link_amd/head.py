"""DenseHead — the siamese pair scorer on the GPU, with the slice of the Keras `Model` API the
reference calls on `SiameseNetwork.siamese_net` (reference code/siamese.py:33-35,57,103,107,116,123,131):
predict / fit / train_on_batch / test_on_batch / get_weights / set_weights / save_weights / load_weights.

All arithmetic happens in libalink_hip.so (head.hip); this file is the Keras-2.1.2 control flow:
validation_split (last 20 % held out BEFORE shuffling), np.random.shuffle of the index array per
epoch, batch-size-weighted epoch means, class_weight -> sample weights, EarlyStopping /
ReduceLROnPlateau bookkeeping.
"""
import ctypes as C

import numpy as np

from . import _abi
from .net_host import Handle


def glorot_uniform(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32)


def to_categorical(y, num_classes=2):
    """keras.utils.to_categorical (reference code/siamese.py:56,100-101)."""
    y = np.asarray(y, dtype="int").ravel()
    out = np.zeros((y.shape[0], num_classes), dtype=np.float32)
    out[np.arange(y.shape[0]), y] = 1.0
    return out


class EarlyStopping(object):
    """keras.callbacks.EarlyStopping (2.1.2) for a monitored quantity that should decrease."""

    def __init__(self, monitor="val_loss", min_delta=0.0, patience=0, verbose=0):
        self.monitor, self.patience, self.verbose = monitor, patience, verbose
        self.min_delta = -abs(min_delta)
        self.wait, self.best, self.stopped_epoch = 0, np.inf, 0

    def on_epoch_end(self, epoch, logs, model):
        current = logs.get(self.monitor)
        if current is None:
            return
        if np.less(current - self.min_delta, self.best):
            self.best, self.wait = current, 0
        else:
            self.wait += 1
            if self.wait >= self.patience:
                self.stopped_epoch = epoch
                model.stop_training = True


class ReduceLROnPlateau(object):
    """keras.callbacks.ReduceLROnPlateau (2.1.2), mode min."""

    def __init__(self, monitor="val_loss", factor=0.1, patience=10, min_lr=0.0, epsilon=1e-4, cooldown=0,
                 verbose=0):
        self.monitor, self.factor, self.patience = monitor, factor, patience
        self.min_lr, self.epsilon, self.cooldown, self.verbose = min_lr, epsilon, cooldown, verbose
        self.wait, self.best, self.cooldown_counter = 0, np.inf, 0

    def on_epoch_end(self, epoch, logs, model):
        logs["lr"] = model.get_lr()
        current = logs.get(self.monitor)
        if current is None:
            return
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.wait = 0
        if np.less(current, self.best - self.epsilon):
            self.best, self.wait = current, 0
        elif not self.cooldown_counter > 0:
            if self.wait >= self.patience:
                old_lr = float(model.get_lr())
                if old_lr > self.min_lr:
                    model.set_lr(max(old_lr * self.factor, self.min_lr))
                    self.cooldown_counter = self.cooldown
                    self.wait = 0
            self.wait += 1


class KerasFitMixin(object):
    """Keras 2.1.2 Model.fit for in-memory arrays on top of train_on_batch / test_on_batch
    (reference code/siamese.py:57).  validation_split holds out the LAST fraction before shuffling;
    np.random.shuffle(index_array) per epoch; epoch logs are batch-size-weighted means."""
    stop_training = False
    # One process per GPU (not in the reference, which is one process on one GPU): with dp_group set, fit() runs its
    # steps through distributed.dp_train_on_batch (replicated below distributed.DP_SHARD_MIN_ROWS rows, sharded with a
    # gradient all-reduce above: dp_mode / dp_exchange) and every epoch's shuffle is rank 0's, so that all ranks hold
    # the same weights afterwards.  alink_loop sets it for the student's fine-tune when the loop runs with `group`.
    dp_group = None          # a torch.distributed ProcessGroup (torch.distributed.group.WORLD for all ranks); None: one process
    dp_mode = "auto"
    dp_exchange = "gather"

    def fit(self, x, y, batch_size=32, epochs=1, verbose=1, callbacks=None, validation_split=0.0, shuffle=True):
        L = np.asarray(x[0], dtype=np.float32)
        R = np.asarray(x[1], dtype=np.float32)
        y = np.asarray(y, dtype=np.float32)
        n_all = L.shape[0]
        if 0.0 < validation_split < 1.0:
            split_at = int(n_all * (1.0 - validation_split))
            vL, vR, vy = L[split_at:], R[split_at:], y[split_at:]
            L, R, y = L[:split_at], R[:split_at], y[:split_at]
        else:
            vL = vR = vy = None
        n = L.shape[0]
        history = {}
        self.stop_training = False
        index_array = np.arange(n)
        step = self.train_on_batch
        group = self.dp_group
        if group is not None:
            import torch.distributed as dist
            if hasattr(self, "grads_tensor"):
                from . import distributed as _D
                step = lambda xb, yb: _D.dp_train_on_batch(self, xb, yb, group=group, mode=self.dp_mode, exchange=self.dp_exchange)
        for epoch in range(epochs):
            if shuffle:
                np.random.shuffle(index_array)
                if group is not None:
                    box = [index_array if dist.get_rank(group) == 0 else None]
                    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0), group=group)
                    index_array = np.array(box[0])
            tot, seen = np.zeros(2), 0
            for s in range(0, n, batch_size):
                ids = index_array[s:s + batch_size]
                out = step([L[ids], R[ids]], y[ids])
                tot += np.asarray(out) * len(ids)
                seen += len(ids)
            logs = {"loss": tot[0] / seen, "acc": tot[1] / seen}
            if vL is not None and len(vy) > 0:
                vt, vs = np.zeros(2), 0
                for s in range(0, len(vy), batch_size):
                    out = self.test_on_batch([vL[s:s + batch_size], vR[s:s + batch_size]], vy[s:s + batch_size])
                    k = len(vy[s:s + batch_size])
                    vt += np.asarray(out) * k
                    vs += k
                logs["val_loss"], logs["val_acc"] = vt[0] / vs, vt[1] / vs
            for cb in (callbacks or []):
                cb.on_epoch_end(epoch, logs, self)
            for k, v in logs.items():
                history.setdefault(k, []).append(v)
            if verbose:
                print("Epoch %d/%d - " % (epoch + 1, epochs) + " - ".join("%s: %.4f" % kv for kv in sorted(logs.items())))
            if self.stop_training:
                break
        return history


def _evaluate(self, x, y, batch_size=32, verbose=0):
    """Keras Model.evaluate: batch-size-weighted means of test_on_batch -> [loss, acc]."""
    L, R, y = np.asarray(x[0], np.float32), np.asarray(x[1], np.float32), np.asarray(y, np.float32)
    tot, seen = np.zeros(2), 0
    for s in range(0, len(y), batch_size):
        k = len(y[s:s + batch_size])
        tot += np.asarray(self.test_on_batch([L[s:s + batch_size], R[s:s + batch_size]], y[s:s + batch_size])) * k
        seen += k
    return list(tot / max(seen, 1))


KerasFitMixin.evaluate = _evaluate


class DenseHead(KerasFitMixin, Handle):
    """abs(l - r) -> Dense(h1, relu) -> Dense(h2, relu) -> Dense(2) -> softmax; BCE + Adadelta.
    out_dim=1 is the baseline scripts' variant: Dense(1, sigmoid) (reference code/siamese3.py:25)."""
    prefix = "alink_head"

    def __init__(self, d_in, h1=512, h2=64, lr=1.0, rho=0.95, eps=1e-8, seed=None, device=None, out_dim=2,
                 compute_dtype="f32"):
        device = self._open(device)                   # None: the current torch device
        torch, self.device = self.torch, "cuda:%d" % device
        self.d_in, self.h1, self.h2, self.out_dim = int(d_in), int(h1), int(h2), int(out_dim)
        with _abi.on_device(device):                  # the handle lives on the device current at create
            self.h = self.lib.alink_head_create_ex(self.d_in, self.h1, self.h2, self.out_dim, lr, rho, eps)
        if not self.h:
            raise _abi.AlinkError("alink_head_create: " + self.lib.alink_last_error().decode())
        self.compute_dtype = "f32"
        self.set_compute_dtype(compute_dtype)
        self.loss = "binary_crossentropy"               # what keras_wrapper reads off model.loss
        self.metrics_names = ["loss", "acc"]
        self.stop_training = False
        rng = np.random.RandomState(seed) if seed is not None else np.random
        # Keras Dense default init: glorot_uniform kernel, zero bias
        self.set_weights([glorot_uniform(rng, d_in, h1), np.zeros(h1, np.float32),
                          glorot_uniform(rng, h1, h2), np.zeros(h2, np.float32),
                          glorot_uniform(rng, h2, self.out_dim), np.zeros(self.out_dim, np.float32)])
        self._metrics = torch.zeros(2, dtype=torch.float32, device=self.device)
        # {loss, accuracy} of a step land in pinned host memory, written by the kernel itself (pinned memory
        # is mapped into the device's address space): the step ends with one stream wait, not a copy
        self._metrics_host = torch.zeros(2, dtype=torch.float32).pin_memory()
        self._metrics_host_ptr = self._metrics_host.data_ptr()
        self._tdev = torch.device(self.device)
        self._stage = {}          # persistent device tensors the host batches are copied into

    def set_compute_dtype(self, compute_dtype):
        """"f32" (default; Keras' floatx, what the reference trains in) or "bf16": mixed precision — f32 master
        weights, gradients and Adadelta state, bf16 GEMM operands (include/alink_hip.h, alink_head_set_compute_dtype)."""
        code = {"f32": _abi.DT_F32, "bf16": _abi.DT_BF16}[compute_dtype]
        _abi.check(self.lib.alink_head_set_compute_dtype(self.h, code), "alink_head_set_compute_dtype")
        self.compute_dtype = compute_dtype

    # -- parameters --------------------------------------------------------------------------------
    def _shapes(self):
        return [(self.d_in, self.h1), (self.h1,), (self.h1, self.h2), (self.h2,), (self.h2, self.out_dim),
                (self.out_dim,)]

    def set_weights(self, ws):
        shapes = self._shapes()
        assert len(ws) == 6, "expected [W1,b1,W2,b2,W3,b3]"
        flat = np.concatenate([np.asarray(w, np.float32).reshape(s).ravel() for w, s in zip(ws, shapes)])
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        _abi.check(self.lib.alink_head_set_params(self.h, _abi.ptr(flat), flat.size), "alink_head_set_params")

    def get_weights(self):
        n = self.lib.alink_head_num_params(self.h)
        flat = np.empty(n, dtype=np.float32)
        _abi.check(self.lib.alink_head_get_params(self.h, _abi.ptr(flat), n), "alink_head_get_params")
        out, o = [], 0
        for s in self._shapes():
            k = int(np.prod(s))
            out.append(flat[o:o + k].reshape(s).copy())
            o += k
        return out

    def get_lr(self):
        return float(self.lib.alink_head_get_lr(self.h))

    def set_lr(self, lr):
        _abi.check(self.lib.alink_head_set_lr(self.h, float(lr)))

    # Keras' own layer / weight names for the graph built at reference code/siamese.py:24-35 (first model
    # of a session): Input, Input, Lambda, Dense x3, Activation
    _KERAS_LAYERS = ["input_1", "input_2", "lambda_1", "dense_1", "dense_2", "dense_3", "activation_1"]

    def save_weights(self, path):
        """Keras Model.save_weights (reference code/siamese.py:121-125): an HDF5 file in Keras 2.1.2's
        layout, written by hdf5_lite.py (a path ending in .npz selects NumPy's format instead)."""
        ws = self.get_weights()
        if path.endswith(".npz"):
            names = ["dense_1/kernel", "dense_1/bias", "dense_2/kernel", "dense_2/bias", "dense_3/kernel",
                     "dense_3/bias"]
            np.savez(path, **dict(zip(names, ws)))
            return
        from . import hdf5_lite
        layers, i = [], 0
        for name in self._KERAS_LAYERS:
            if name.startswith("dense"):
                layers.append((name, [("%s/kernel:0" % name, ws[i]), ("%s/bias:0" % name, ws[i + 1])]))
                i += 2
            else:
                layers.append((name, []))
        hdf5_lite.save_keras_weights(path, layers)

    def load_weights(self, path):
        """Keras Model.load_weights (code/siamese.py:116), topological: the weighted layers of the file,
        in file order, must match this model's (keras/engine/topology.py load_weights_from_hdf5_group)."""
        with open(path, "rb") as f:
            magic = f.read(8)
        if magic[:4] == b"PK\x03\x04":
            with np.load(path) as z:
                names = ["dense_1/kernel", "dense_1/bias", "dense_2/kernel", "dense_2/bias", "dense_3/kernel",
                         "dense_3/bias"]
                self.set_weights([z[n] for n in names])
            return
        from . import hdf5_lite
        layers = [(n, ws) for n, ws in hdf5_lite.load_keras_weights(path) if ws]
        if len(layers) != 3:
            raise ValueError("You are trying to load a weight file containing %d layers into a model with 3 layers."
                             % len(layers))
        flat = [a for _, ws in layers for _, a in ws]
        for a, shp in zip(flat, self._shapes()):
            if tuple(a.shape) != tuple(shp):
                raise ValueError("weight of shape %s in the file does not fit %s" % (a.shape, shp))
        self.set_weights(flat)

    # -- device helpers ----------------------------------------------------------------------------
    def _dev(self, a, dtype=None):
        torch = self.torch
        if isinstance(a, torch.Tensor):
            t = a.to(self.device)
            if dtype is not None and t.dtype != dtype:
                t = t.to(dtype)
            return t.contiguous()
        a = np.ascontiguousarray(a, dtype=np.float32 if dtype in (None, torch.float32) else np.int32)
        return torch.from_numpy(a).to(self.device)

    def grads_tensor(self, with_metrics=False):
        """torch view-less alias of the flat gradient buffer (for torch.distributed.all_reduce); with_metrics
        appends the 4 spare floats that follow it (slot 0 / 1: loss, accuracy of a data-parallel step)."""
        return self._alias(self.lib.alink_head_grads_dev(self.h), 4 if with_metrics else 0)

    def params_tensor(self):
        return self._alias(self.lib.alink_head_params_dev(self.h))

    def _alias(self, devptr, extra=0):
        torch = self.torch
        n = self.lib.alink_head_num_params(self.h) + extra

        class _CAI(object):  # __cuda_array_interface__ holder
            pass
        holder = _CAI()
        holder.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (int(devptr), False),
                                           "version": 2, "strides": None}
        t = torch.as_tensor(holder, device=self.device)
        t._alink_owner = self
        return t

    # -- inference ---------------------------------------------------------------------------------
    def predict_device(self, L, R, li=None, ri=None, out=None):
        torch = self.torch
        L, R = self._dev(L), self._dev(R)
        if li is not None:
            li, ri = self._dev(li, torch.int32), self._dev(ri, torch.int32)
            P = li.numel()
        else:
            assert L.shape == R.shape
            P = L.shape[0]
        assert L.shape[1] == self.d_in and R.shape[1] == self.d_in
        if out is None:
            out = torch.empty((P, self.out_dim), dtype=torch.float32, device=self.device)
        if P == 0:
            return out
        _abi.check(self.lib.alink_head_forward(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(li), _abi.ptr(ri), P,
                                               _abi.ptr(out), _abi.current_stream(self.device)), "alink_head_forward")
        return out

    def expected_gradient_length_device(self, L, R, li=None, ri=None, want=("egl",)):
        """EXTENSION (egl.py): expected gradient length, probabilities and gradient embeddings of the pairs
        (L[n], R[n]) or (L[li[n]], R[ri[n]]) on the device -> {name: CUDA tensor}; egl.expected_gradient_length_device's."""
        from . import egl as _egl
        return _egl.expected_gradient_length_device(self, L, R, li, ri, want=want)

    def feature_mix_device(self, L, R, anchors, li=None, ri=None, eps=0.2, want=("probs", "flip")):
        """EXTENSION (alfamix.py): ALFA-Mix's feature mix of the pairs (L[n], R[n]) or (L[li[n]], R[ri[n]])
        towards the (A, D) anchors on the device: the probabilities, the mask of anchors that flip the decision, and on request
        the mixed rows and their probabilities -> {name: CUDA tensor}; alfamix.feature_mix_device's."""
        from . import alfamix as _alfamix
        return _alfamix.feature_mix_device(self, L, R, anchors, li, ri, eps=eps, want=want)

    def badge_device(self, L, R, li=None, ri=None, n_instances=1, uniforms=None, seed=None):
        """EXTENSION (badge.py): a BADGE batch — k-means++ seeding over the gradient embeddings of the pairs
        (L[n], R[n]) or (L[li[n]], R[ri[n]]) on the device -> (idx int32 (k,), potential float64 (k,)); badge.badge_device's."""
        from . import badge as _badge
        return _badge.badge_device(self, L, R, li, ri, n_instances=n_instances, uniforms=uniforms, seed=seed)

    def bait_device(self, L, R, li=None, ri=None, labelled=None, n_instances=1, lam=1.0, over=2):
        """EXTENSION (bait.py): a BAIT batch — Fisher-information greedy selection over the last layer's rank-one
        Fisher factors of the pairs (L[n], R[n]) or (L[li[n]], R[ri[n]]) on the device -> (idx int32 (k,), score float32 (k,));
        bait.bait_device's."""
        from . import bait as _bait
        return _bait.bait_device(self, L, R, li, ri, labelled=labelled, n_instances=n_instances, lam=lam, over=over)

    def predict(self, X, batch_size=1024, verbose=0):
        """Keras Model.predict([L, R]) (reference code/siamese.py:131).  batch_size is accepted for
        API compatibility; the kernel tiles the pairs itself."""
        L, R = X
        as_torch = isinstance(L, self.torch.Tensor)
        out = self.predict_device(L, R)
        return out if as_torch else out.cpu().numpy()

    # -- training ----------------------------------------------------------------------------------
    @staticmethod
    def _sample_weights(y, class_weight, sample_weight):
        if sample_weight is not None:
            return np.asarray(sample_weight, np.float32)
        if class_weight is not None:
            ya = np.asarray(y)
            # keras/engine/training.py _standardize_weights: argmax for one-hot targets, the value itself for (n, 1)
            cls = ya.argmax(axis=1) if ya.shape[1] > 1 else ya[:, 0].astype(int)
            missing = sorted(set(int(c) for c in cls) - set(class_weight))
            if missing:                 # Keras raises here too instead of silently shortening the vector
                raise ValueError("class_weight must contain all classes in the data; missing %s" % missing)
            return np.asarray([class_weight[c] for c in cls], dtype=np.float32)
        return None

    def _staged(self, key, a):
        """Device float32 tensor holding `a` at an address that stays the same from call to call."""
        torch = self.torch
        if isinstance(a, torch.Tensor):
            if a.dtype is torch.float32 and a.is_cuda and a.is_contiguous() and a.device == self._tdev:
                return a                                                  # the caller's own buffer, as it is
            return a.to(self.device, torch.float32).contiguous()
        arr = np.ascontiguousarray(a, dtype=np.float32)
        buf = self._stage.get((key, arr.shape))
        if buf is None:
            buf = self._stage[(key, arr.shape)] = torch.empty(arr.shape, dtype=torch.float32, device=self.device)
        buf.copy_(torch.from_numpy(arr))
        return buf

    def fit(self, x, y, batch_size=32, epochs=1, verbose=1, callbacks=None, validation_split=0.0, shuffle=True):
        """KerasFitMixin.fit with the training set RESIDENT on the device: the arrays go up once, every step gathers its rows
        by index on the device and writes its {loss, accuracy} into a per-epoch device buffer that is read back once per
        epoch — the same kernels on the same batches in the same order as the step-by-step form (bit-identical weights and
        logs: tests/test_gpu_head.py), without an upload, a host gather and a synchronisation per step (a fine-tune of the
        A-LINK loop, ~150 steps of 0.04 ms: 26 -> ~8 ms).  Sharded data-parallel steps (dp_group with a batch of
        DP_SHARD_MIN_ROWS rows or more) keep the generic form."""
        from . import distributed as _D
        bs = int(batch_size)
        if self.dp_group is not None and not (self.dp_mode == "replicated" or (self.dp_mode == "auto" and bs < _D.DP_SHARD_MIN_ROWS)):
            return super(DenseHead, self).fit(x, y, batch_size, epochs, verbose, callbacks, validation_split, shuffle)
        if type(self).train_on_batch is not DenseHead.train_on_batch or type(self).test_on_batch is not DenseHead.test_on_batch:
            # a subclass (or an instrumented copy) that overrides a step must see every step: the generic form calls them
            return super(DenseHead, self).fit(x, y, batch_size, epochs, verbose, callbacks, validation_split, shuffle)
        torch = self.torch
        L, R, Y = self._dev(x[0]), self._dev(x[1]), self._dev(np.asarray(y, dtype=np.float32) if not isinstance(y, torch.Tensor) else y)
        n_all = L.shape[0]
        if 0.0 < validation_split < 1.0:
            split_at = int(n_all * (1.0 - validation_split))
            vL, vR, vY = L[split_at:], R[split_at:], Y[split_at:]
            L, R, Y = L[:split_at], R[:split_at], Y[:split_at]
        else:
            vL = vR = vY = None
        n = L.shape[0]
        history = {}
        self.stop_training = False
        index_array = np.arange(n)
        group = self.dp_group
        st = torch.cuda.current_stream(self._tdev)
        starts = list(range(0, n, bs))
        sizes = np.asarray([min(bs, n - s0) for s0 in starts], np.float64)
        vstarts = list(range(0, 0 if vY is None else len(vY), bs))
        vsizes = np.asarray([min(bs, len(vY) - s0) for s0 in vstarts], np.float64) if vstarts else None
        for epoch in range(epochs):
            if shuffle:
                np.random.shuffle(index_array)
                if group is not None:
                    import torch.distributed as dist
                    box = [index_array if dist.get_rank(group) == 0 else None]
                    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0), group=group)
                    index_array = np.array(box[0])
            idx = torch.from_numpy(index_array).to(self.device)
            M = torch.zeros((len(starts) + len(vstarts), 4), dtype=torch.float32, device=self.device)
            # (a step's gathered operands need no pinning: torch's allocator is stream-ordered, and everything here runs on ONE
            # stream — a block freed by Python is reused only by work queued behind the launch that reads it; ADVICE r5: the
            # list kept here until round 6 held a second copy of the training set per epoch)
            for k, s0 in enumerate(starts):
                ids = idx[s0:s0 + bs]
                Lb, Rb, Yb = L.index_select(0, ids), R.index_select(0, ids), Y.index_select(0, ids)
                rc = self.lib.alink_head_train_step(self.h, Lb.data_ptr(), Rb.data_ptr(), Yb.data_ptr(), None, Lb.shape[0], 0.0, 1,
                                                    M[k].data_ptr(), st.cuda_stream)
                if rc:
                    _abi.check(rc, "alink_head_train_step")
            for k, s0 in enumerate(vstarts):
                a, b, c = vL[s0:s0 + bs].contiguous(), vR[s0:s0 + bs].contiguous(), vY[s0:s0 + bs].contiguous()
                _abi.check(self.lib.alink_head_eval(self.h, _abi.ptr(a), _abi.ptr(b), _abi.ptr(c), a.shape[0],
                                                    C.c_void_p(M[len(starts) + k].data_ptr()), C.c_void_p(st.cuda_stream)), "alink_head_eval")
            m = M.cpu().numpy().astype(np.float64)                # one read-back (and synchronisation) per epoch
            tr = m[:len(starts), :2]
            # the same accumulation as the step-by-step form: sum of per-step value x size, in step order
            tot = np.zeros(2)
            for k in range(len(starts)):
                tot += tr[k] * sizes[k]
            logs = {"loss": tot[0] / n, "acc": tot[1] / n}
            if vstarts:
                vt = np.zeros(2)
                for k in range(len(vstarts)):
                    vt += m[len(starts) + k, :2] * vsizes[k]
                logs["val_loss"], logs["val_acc"] = vt[0] / len(vY), vt[1] / len(vY)
            for cb in (callbacks or []):
                cb.on_epoch_end(epoch, logs, self)
            for kk, v in logs.items():
                history.setdefault(kk, []).append(v)
            if verbose:
                print("Epoch %d/%d - " % (epoch + 1, epochs) + " - ".join("%s: %.4f" % kv for kv in sorted(logs.items())))
            if self.stop_training:
                break
        return history

    def train_on_batch(self, x, y, class_weight=None, sample_weight=None, metrics_out=None):
        """metrics_out (not in Keras): a device float32 tensor of >= 2 elements that receives {loss, accuracy} INSTEAD of the
        return value — the step is then only enqueued (no synchronisation, returns None): a caller that needs the numbers
        per epoch, not per step (customTrainModel with verbose = 0), reads a whole block of them back at once."""
        L, R = self._staged("L", x[0]), self._staged("R", x[1])
        yd = self._staged("y", y)
        sw = self._sample_weights(y, class_weight, sample_weight)
        swd = self._staged("sw", sw) if sw is not None else None
        n = L.shape[0]
        st = self.torch.cuda.current_stream(self._tdev)        # looked up once: launch on it, then wait on it
        rc = self.lib.alink_head_train_step(self.h, L.data_ptr(), R.data_ptr(), yd.data_ptr(),
                                            swd.data_ptr() if swd is not None else None, n, 0.0, 1,
                                            self._metrics_host_ptr if metrics_out is None else metrics_out.data_ptr(), st.cuda_stream)
        if rc:
            _abi.check(rc, "alink_head_train_step")
        if metrics_out is not None:
            return None
        st.synchronize()
        return self._metrics_host.tolist()

    # -- the model's side of distributed.dp_train_on_batch (sharded mode) -------------------------------------------
    def dp_begin(self, n, group):
        return None

    def dp_local_grads(self, x, y, w_all, lo, hi, n, grad_scale, m, ctx):
        """gradients (left in grads_tensor()) and {loss x grad_scale sum, accuracy mean} (into m) of rows lo : hi"""
        take = lambda a: a[lo:hi] if hasattr(a, "shape") else np.asarray(a)[lo:hi]
        L, R = self._dev(take(x[0])), self._dev(take(x[1]))
        yd, swd = self._dev(take(y)), (None if w_all is None else self._dev(w_all[lo:hi]))
        _abi.check(self.lib.alink_head_train_step(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), _abi.ptr(swd),
                                                  hi - lo, grad_scale, 0, _abi.ptr(m), _abi.current_stream(self.device)),
                   "alink_head_train_step")

    def dp_apply(self):
        _abi.check(self.lib.alink_head_apply_update(self.h, _abi.current_stream(self.device)), "alink_head_apply_update")

    def input_gradients(self, L, R, y, sample_weight=None):
        """EXTENSION (FGSM / PGD): d(loss)/dL, d(loss)/dR of the Keras loss of this batch (mean over the
        batch), parameters untouched.  L, R: (n, d_in) CUDA float32; y: (n, out_dim) targets."""
        torch = self.torch
        L, R, yd = self._dev(L), self._dev(R), self._dev(y)
        swd = None if sample_weight is None else self._dev(np.asarray(sample_weight, dtype=np.float32))
        n = L.shape[0]
        dL, dR = torch.empty_like(L), torch.empty_like(R)
        # the input-gradient kernels are float32 only; a head in the bf16 compute mode (BASELINE configs[4]: gradient-attack
        # noise + bf16 fine-tune in ONE loop) differentiates its float32 MASTER weights for the call — an attack needs a
        # direction, and the masters are what the bf16 copies are rounded from — and returns to its mode afterwards
        quantised = self.compute_dtype == "bf16"
        if quantised:
            self.set_compute_dtype("f32")
        try:
            _abi.check(self.lib.alink_head_train_step_input_grads(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), _abi.ptr(swd), n, 0.0, 0,
                                                                  _abi.ptr(dL), _abi.ptr(dR), None, _abi.ptr(self._metrics),
                                                                  _abi.current_stream(self.device)), "alink_head_train_step_input_grads")
        finally:
            if quantised:
                self.set_compute_dtype("bf16")
        return dL, dR

    def test_on_batch(self, x, y, metrics_out=None):
        if metrics_out is not None:          # enqueue only (see train_on_batch): operands in buffers that outlive the call
            L, R, yd = self._staged("vL", x[0]), self._staged("vR", x[1]), self._staged("vy", y)
            _abi.check(self.lib.alink_head_eval(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), L.shape[0],
                                                C.c_void_p(metrics_out.data_ptr()), _abi.current_stream(self.device)), "alink_head_eval")
            return None
        L, R = self._dev(x[0]), self._dev(x[1])
        yd = self._dev(y)
        _abi.check(self.lib.alink_head_eval(self.h, _abi.ptr(L), _abi.ptr(R), _abi.ptr(yd), L.shape[0],
                                            _abi.ptr(self._metrics_host), _abi.current_stream(self.device)), "alink_head_eval")
        self.torch.cuda.current_stream(self.device).synchronize()
        return self._metrics_host.tolist()


def committee_predict_device(heads, L, R, li=None, ri=None):
    """Bagging.predict on device: sum of member softmaxes / M (reference code/committee.py:13-20).
    L / R: one pair of matrices shared by every member, or a list with one matrix per member (members with
    different feature extractors) — then li / ri index every member's own matrices."""
    h0 = heads[0]
    torch = h0.torch
    per_member = isinstance(L, (list, tuple))
    if per_member:
        if len(L) != len(heads) or len(R) != len(heads):
            raise ValueError("%d members but %d / %d feature matrices" % (len(heads), len(L), len(R)))
        Ls, Rs = [h0._dev(a) for a in L], [h0._dev(a) for a in R]
        if any(a.shape != Ls[0].shape for a in Ls) or any(a.shape != Rs[0].shape for a in Rs):
            raise ValueError("per-member feature matrices must have one shape")
        L, R = Ls[0], Rs[0]
    else:
        L, R = h0._dev(L), h0._dev(R)
    if li is not None:
        li, ri = h0._dev(li, torch.int32), h0._dev(ri, torch.int32)
        P = li.numel()
    else:
        P = L.shape[0]
    out = torch.empty((P, 2), dtype=torch.float32, device=h0.device)
    if P == 0:
        return out
    arr = (C.c_void_p * len(heads))(*[h.h for h in heads])
    if per_member:
        la = (C.c_void_p * len(heads))(*[a.data_ptr() for a in Ls])
        ra = (C.c_void_p * len(heads))(*[a.data_ptr() for a in Rs])
        _abi.check(h0.lib.alink_committee_forward_multi(arr, len(heads), la, ra, _abi.ptr(li), _abi.ptr(ri), P,
                                                        _abi.ptr(out), _abi.current_stream(h0.device)),
                   "alink_committee_forward_multi")
        return out
    _abi.check(h0.lib.alink_committee_forward(arr, len(heads), _abi.ptr(L), _abi.ptr(R), _abi.ptr(li), _abi.ptr(ri),
                                              P, _abi.ptr(out), None, _abi.current_stream(h0.device)), "alink_committee_forward")
    return out


def committee_member_probs_device(heads, L, R, li=None, ri=None):
    """Every member's own probabilities, WITHOUT the mean: (M, P, out_dim) CUDA float32, slab m written in place by
    heads[m].predict_device (alink_head_forward) — what the query-by-committee measures need, which the mean of
    committee_predict_device has already lost (disagreement.score_members_device).  L / R: shared matrices, or a list
    with one matrix per member, as committee_predict_device takes them."""
    h0 = heads[0]
    torch = h0.torch
    if any(h.out_dim == 1 for h in heads):
        raise TypeError("committee disagreement needs class probabilities: a one-column (out_dim == 1) member has no vote to count")
    if any(h.out_dim != h0.out_dim for h in heads):
        raise ValueError("committee members differ in out_dim")
    per_member = isinstance(L, (list, tuple))
    if per_member and (len(L) != len(heads) or len(R) != len(heads)):
        raise ValueError("%d members but %d / %d feature matrices" % (len(heads), len(L), len(R)))
    if li is not None:
        li, ri = h0._dev(li, torch.int32), h0._dev(ri, torch.int32)
        P = li.numel()
    else:
        P = len(L[0] if per_member else L)
    out = torch.empty((len(heads), P, h0.out_dim), dtype=torch.float32, device=h0.device)
    for m, h in enumerate(heads):
        h.predict_device(L[m] if per_member else L, R[m] if per_member else R, li, ri, out=out[m])
    return out
