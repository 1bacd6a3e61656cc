"""IRBackbone — host-side owner of one alink_backbone_t handle (include/alink_hip.h).

Device memory (inputs, outputs, workspace) is allocated through torch; the arithmetic runs in
libalink_hip.so.  Mirrors what face_model.get_model builds (reference code/face_model.py:28-41) but
binds a *batched* executor: the reference binds batch = 1 (code/face_model.py:39).
"""
import ctypes as C

import numpy as np

from . import _abi
from . import weights as W
from .net_host import F16_STORAGE, ImageNet


class IRBackbone(ImageNet):
    prefix = "alink_backbone"
    DTYPES = {"bf16": _abi.DT_BF16, "f16": _abi.DT_F16, "f32": _abi.DT_F32, "f16x2": _abi.DT_F16X2}

    def __init__(self, params, image_size=(112, 112), emb=512, dtype="bf16", device=None, max_batch=292,
                 widths=W.WIDTHS, streams=2, shards_per_call=None, bn_eps=2e-5, enable_grad=False,
                 small_batch_split=False, lazy_range_check=False):
        self.device = self._open(device)              # None: the current torch device
        self._embed = self.lib.alink_embed
        self.units = W.infer_units(params)
        self.emb = emb
        self.image_size = tuple(image_size)
        # 292 images per launch: 292 x 196 pixels / 224 per workgroup x 2 channel halves = 511 workgroups of the
        # 14-wide convolutions for the chip's 512 slots (1022 / 1024 at 28 wide) — a lone 256-image launch leaves 64 idle
        self.max_batch = int(max_batch)
        cfg = _abi.IRCfg()
        cfg.units[:] = list(self.units)
        cfg.widths[:] = list(widths)
        cfg.height, cfg.width = int(image_size[0]), int(image_size[1])
        cfg.emb = emb
        cfg.bn_eps = float(bn_eps)
        self.grad_enabled = bool(enable_grad)
        # dtype "auto": float16 storage (11 significant bits: 1 - cos ~4e-6 against the f32 arithmetic at IR-100 depth,
        # and selection sets that follow it: DESIGN.md §5) when the network's activations fit its range, else bfloat16
        # (8 significant bits, f32's range: 1 - cos ~3e-4).  The range is probed on three images at build time (uniform
        # noise, all 0, all 255); later inputs that leave it raise AlinkError in embed (never NaN embeddings).
        #
        # dtype "f16x2" — SPLIT PRECISION, the mode for selection: every activation and folded weight is an f16 pair
        # hi + lo (22 significant bits) under a power-of-two scale per tensor, three products on the f16 matrix cores
        # into f32 accumulators.  The accuracy of the float32 mode (active-learning selection sets identical to the f32
        # arithmetic: DESIGN.md §5) at about a third of the bf16 rate.  Scales are calibrated on the same three probe
        # images plus whatever `calibrate()` is given later.  For FIXED scales an image embeds to the same bits whatever
        # batch it arrives in; a different calibration moves embeddings by ~2e-7 (the lo halves of values 2^13 below a
        # tensor's maximum are subnormal f16 and round differently) — far below the mode's error, not zero: share scales
        # with state() / load_state().  A batch that leaves the range (32x above the calibration images' largest
        # activation) is re-calibrated on (every chunk of it) and re-run, which changes the scales from then on.
        self._shards_fixed = None if shards_per_call is None else int(shards_per_call)
        self.lazy_range_check = bool(lazy_range_check)
        order = ["f16", "bf16"] if dtype == "auto" else [dtype]
        for dt in order:
            cfg.dtype = self.DTYPES[dt]
            self.dtype = dt
            self._build(cfg, params, small_batch_split, enable_grad)
            if dt == "f16x2":
                self.calibrate(self.probe_images())
            if dtype != "auto" or dt == "bf16" or self._range_probe_ok():
                break
            self._destroy()
        # shards_per_call: image shards ONE alink_embed call is split into on the library's internal streams.  None
        # (default) = 2 for a call that is alone on its stream and has >= 192 images — two half-launches de-phase each
        # other's prologue / epilogue bursts: IR-50, one 256-image batch per step 65.9k -> 72.0k embeddings/s, IR-100 at
        # 292 images +1.5 % — and 1 for the chunks of a multi-stream call, which already overlap (sharding those costs 11 %).
        self._set_shards(self._shards_fixed or 1)
        # Inputs larger than max_batch are cut into max_batch-image chunks issued round-robin on
        # `streams` side streams (each with its own workspace) and joined once at the end: chunks are
        # independent, and de-synchronising them lets the HBM bursts of one chunk's tiles overlap the
        # matrix-core phases of the others (+8...10 % measured on r100).  Two streams since the front of the network is
        # one persistent launch that owns every CU while it runs (front_c64.hip): 46.1 k against 44.8 k embeddings/s with
        # four (rounds 1-2, tile kernels throughout: four).
        self.n_streams = max(1, int(streams))
        self._side = None
        self._upload = None
        self.ws.slots.clear()                         # the probe / calibration workspace of the build is not kept

    def _build(self, cfg, params, small_batch_split, enable_grad):
        self._create(self.device, C.byref(cfg))
        if small_batch_split:      # latency mode: batches <= 32 split their convolutions over K (not bit-equal to fused)
            _abi.check(self.lib.alink_backbone_set_small_batch_split(self.h, 1), "alink_backbone_set_small_batch_split")
        if enable_grad:
            _abi.check(self.lib.alink_backbone_enable_grad(self.h), "alink_backbone_enable_grad")
        self.load_tensors(params, "checkpoint is")
        self._shards_now = None                       # a new handle: its shard count is not set yet

    def calibrate(self, x, merge=False):
        """dtype 'f16x2': choose the per-tensor power-of-two scales from these images (CUDA tensor or host array in any
        accepted layout; ALL of them, max_batch at a time: the first chunk sets the scales unless merge, every further
        chunk only lowers them).  merge=True only ever lowers a scale.  Embeddings are bit-reproducible for FIXED
        scales: share them with state() / load_state() (checkpoints, the ranks of a job)."""
        if isinstance(x, np.ndarray):
            x = self.torch.from_numpy(np.ascontiguousarray(x if x.dtype == np.uint8 else x.astype(np.float32)))
        layout, fn = self._layout_of(x, self.image_size), self.lib.alink_backbone_calibrate
        self._calibrate_chunks(x, merge, lambda xc, n, ws, wsb, m, st: fn(self.h, _abi.ptr(xc), layout, n, ws, wsb, m, st))

    def set_products(self, n):
        """dtype 'f16x2': matrix-core products per multiplication for the launches that follow — 3 = the exact mode
        (default), 1 = X_hi W_hi alone, the screening form on this same handle (include/alink_hip.h)."""
        _abi.check(self.lib.alink_backbone_set_products(self.h, int(n)), "alink_backbone_set_products")

    def screening_view(self):
        """An object with this backbone's embed / embed_device that runs them in the ONE-product screening form (same
        weights, scales and workspace; products are switched back to 3 after every call).  What screen-then-settle
        takes as its screening model when the exact model is this handle: no second copy of the network, no float16
        range to leave."""
        if self.dtype != "f16x2":
            raise _abi.AlinkError("screening_view is the one-product form of dtype='f16x2'")
        return _ScreeningView(self)

    def _identity(self):
        return {"units": [int(u) for u in self.units], "image_size": [int(v) for v in self.image_size]}

    def _misfit(self, st):
        return ("calibration state of a %s %s network at %s does not fit this %s %s network at %s"
                % (st.get("dtype"), st.get("units"), st.get("image_size"), self.dtype, list(self.units), list(self.image_size)))

    def _range_probe_ok(self):
        torch = self.torch
        x = self.probe_images()
        saved, self.dtype = self.dtype, "probe"       # _checked must not raise here
        self._side, self._upload, self.n_streams = None, None, 1
        out = self.embed_device(x)
        self.dtype = saved
        return bool(torch.isfinite(out).all())

    def _set_shards(self, n):
        if n != self._shards_now:
            _abi.check(self.lib.alink_backbone_set_streams(self.h, int(n)), "alink_backbone_set_streams")
            self._shards_now = n

    @staticmethod
    def _layout_of(x, image_size):
        if x.ndim != 4:
            raise ValueError("expected a 4-d batch of images, got shape %s" % (tuple(x.shape),))
        h, w = image_size
        is_u8 = str(x.dtype) in ("uint8", "torch.uint8")
        if tuple(x.shape[1:]) == (h, w, 3):
            return _abi.LAYOUT_NHWC_U8 if is_u8 else _abi.LAYOUT_NHWC_F32
        if tuple(x.shape[1:]) == (3, h, w) and not is_u8:
            return _abi.LAYOUT_NCHW_F32
        raise ValueError("images of shape %s do not match (N,%d,%d,3) / (N,3,%d,%d)" % (tuple(x.shape), h, w, h, w))

    def _check_input(self, x):
        return self._layout_of(x, self.image_size)

    def embed_device(self, x, out=None, _retry=True):
        """x: CUDA tensor (N,H,W,3) f32|u8 or (N,3,H,W) f32, contiguous.  Returns (N, emb) f32 CUDA."""
        torch = self.torch
        layout = self._layout_of(x, self.image_size)
        if self.lazy_range_check and self.dtype in F16_STORAGE and self.range_left(reset=False):
            self.range_left()
            raise _abi.AlinkError("an earlier forward left the float16 range (lazy_range_check): its embeddings are not finite")
        if not x.is_contiguous():
            x = x.contiguous()
        n = x.shape[0]
        if out is None:
            out = torch.empty((n, self.emb), dtype=torch.float32, device=x.device)
        nchunks = (n + self.max_batch - 1) // self.max_batch
        if nchunks == 1 or self.n_streams == 1:
            st = _abi.current_stream(self.device)
            for i in range(0, n, self.max_batch):
                m = min(self.max_batch, n - i)
                self._set_shards(self._shards_fixed or (2 if m >= 192 else 1))
                ws, wsb = self.ws.get(m)
                _abi.check(self._embed(self.h, _abi.ptr(x[i:i + m]), layout, m, _abi.ptr(out[i:i + m]), ws, wsb, st), "alink_embed")
            return self._checked(out, x if _retry else None)
        if self._side is None:
            self._side = [torch.cuda.Stream(device=x.device) for _ in range(self.n_streams)]
        cur = torch.cuda.current_stream(x.device)
        ready = torch.cuda.Event()
        ready.record(cur)                       # inputs (and `out`) are valid in caller-stream order
        used = min(self.n_streams, nchunks)
        self._set_shards(self._shards_fixed or 1)
        for s in self._side[:used]:
            s.wait_event(ready)
        for j, i in enumerate(range(0, n, self.max_batch)):
            m = min(self.max_batch, n - i)
            slot = j % used
            ws, wsb = self.ws.get(m, slot + 1)
            _abi.check(self._embed(self.h, _abi.ptr(x[i:i + m]), layout, m, _abi.ptr(out[i:i + m]), ws, wsb,
                                   self._side[slot].cuda_stream), "alink_embed")
        for s in self._side[:used]:
            done = torch.cuda.Event()
            done.record(s)
            cur.wait_event(done)                # results are valid in caller-stream order
        return self._checked(out, x if _retry else None)

    # -- input gradient (FGSM / PGD extension) --------------------------------------------------------
    def embed_with_cache(self, x):
        """Forward on <= max_batch images keeping what input_gradient needs.  x: CUDA float32 NHWC/NCHW."""
        layout, x, n, out, ws, wsb = self._cache_args(x, self.emb)
        _abi.check(self.lib.alink_embed_cached(self.h, _abi.ptr(x), layout, n, _abi.ptr(out), ws, wsb,
                                               _abi.current_stream(self.device)), "alink_embed_cached")
        self._cached = (n, layout, out)
        return out

    def input_gradient(self, demb):
        """d(loss)/d(pixels) for the batch of the last embed_with_cache, given demb = d(loss)/d(embedding)
        (n, emb) float32 CUDA.  Same layout as the forward input."""
        (n, layout, emb), demb, ws, wsb = self._grad_args(demb, self.emb)
        h, w = self.image_size
        shape = (n, h, w, 3) if layout == _abi.LAYOUT_NHWC_F32 else (n, 3, h, w)
        dpix = self.torch.empty(shape, dtype=self.torch.float32, device=demb.device)
        _abi.check(self.lib.alink_embed_input_grad(self.h, _abi.ptr(demb), _abi.ptr(emb), layout, n, _abi.ptr(dpix), ws, wsb,
                                                   _abi.current_stream(self.device)), "alink_embed_input_grad")
        return dpix

    def embed(self, x):
        """numpy in -> numpy out (the reference's calling convention: host arrays, code/siamese.py:234);
        torch CUDA tensor in -> torch CUDA tensor out."""
        torch = self.torch
        if isinstance(x, np.ndarray):
            if x.dtype != np.uint8:
                x = np.ascontiguousarray(x, dtype=np.float32)
            x = np.ascontiguousarray(x)
            dev = "cuda:%d" % self.device
            n = x.shape[0]
            group = self.max_batch * self.n_streams
            if n <= group:
                return self.embed_device(torch.from_numpy(x).to(dev)).cpu().numpy()
            # Large host arrays go up in groups of max_batch * streams images: the (host-blocking) upload of a
            # group overlaps the launches already queued for the one before, and the device never holds
            # more than two groups of pixels (a 100k-image pool is 15 GB of float32).
            out = torch.empty((n, self.emb), dtype=torch.float32, device=dev)
            if self._upload is None:
                self._upload = torch.cuda.Stream(device=dev)
            cur = torch.cuda.current_stream(self.device)
            for i in range(0, n, group):
                with torch.cuda.stream(self._upload):        # not ordered behind the compute already queued
                    xd = torch.from_numpy(x[i:i + group]).to(dev)
                    up = torch.cuda.Event()
                    up.record(self._upload)
                cur.wait_event(up)
                xd.record_stream(cur)                         # allocated on the upload stream, consumed in `cur` order
                self.embed_device(xd, out=out[i:i + group])
            return out.cpu().numpy()
        return self.embed_device(x)

    def profile(self, x):
        """One profiled forward: list of (kind, ms, flops) per launch (HIP events on the stream)."""
        torch = self.torch
        layout = self._layout_of(x, self.image_size)
        n = x.shape[0]
        assert n <= self.max_batch
        out = torch.empty((n, self.emb), dtype=torch.float32, device=x.device)
        ws, wsb = self.ws.get(n)
        cap = 1024
        ms = (C.c_float * cap)()
        fl = (C.c_double * cap)()
        kd = (C.c_int * cap)()
        nl = C.c_int(cap)
        _abi.check(self.lib.alink_embed_profile(self.h, _abi.ptr(x), layout, n, _abi.ptr(out), ws, wsb,
                                                _abi.current_stream(self.device), ms, fl, kd, C.byref(nl)), "alink_embed_profile")
        return [(kd[i], ms[i], fl[i]) for i in range(nl.value)]


class _ScreeningView(object):
    def __init__(self, bb):
        self.bb = bb
        self.dtype = "f16x2/1"
        self.max_batch, self.image_size, self.emb, self.device = bb.max_batch, bb.image_size, bb.emb, bb.device

    def _run(self, fn, *a, **k):
        self.bb.set_products(1)
        try:
            return fn(*a, **k)
        finally:
            self.bb.set_products(3)

    def embed_device(self, x, out=None):
        return self._run(self.bb.embed_device, x, out=out)

    def embed(self, x):
        return self._run(self.bb.embed, x)
