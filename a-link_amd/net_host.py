"""net_host — the Python plumbing the owners of a C handle share, as csrc/net_host.h is the C++ side's: aligned scratch, the
grow-only workspace cache, the GPU check, `Handle` (create / destroy of one handle of a `prefix` family) and `ImageNet`, what
the alink_backbone_* / alink_resnet50_* / alink_vgg16_* families make uniform (include/alink_hip.h): checkpoint walk, probe
images, calibration state, the calibrate chunk loop, the float16 range rule and the arguments of the gradient pass."""
import ctypes as C

import numpy as np

from . import _abi

F16_STORAGE = ("f16", "f16x2")          # the dtypes whose activations are stored with 5 exponent bits
RANGE_TEXT = ("activations exceeded the float16 range in this network: use dtype='bf16' (or dtype='f16x2', calibrated on "
              "images like these)")


def aligned_scratch(nbytes, device):
    """(tensor, pointer, usable_bytes): uint8 scratch on `device` and its first 256-byte-aligned address — the alignment every
    workspace / scratch argument of the library asks for (include/alink_hip.h)."""
    import torch
    t = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    off = (-t.data_ptr()) % 256
    return t, t.data_ptr() + off, t.numel() - off


class Workspace(object):
    """Grow-only scratch per slot (0: the caller's stream, 1..: side streams, "grad": the gradient cache).
    bytes_for(n, slot): the bytes `n` images need there; device: a torch device."""

    def __init__(self, bytes_for, device):
        self.bytes_for, self.device = bytes_for, device
        self.slots = {}                               # slot -> (tensor, pointer, usable_bytes, images it holds)

    def get(self, n, slot=0):
        """(pointer, usable_bytes) of a workspace for n images; allocates only when n exceeds what the slot holds"""
        cur = self.slots.get(slot)
        if cur is None or n > cur[3]:
            nbytes = self.bytes_for(n, slot)
            self.slots[slot] = cur = None             # release the smaller one first: ResNet-50's gradient cache is ~18 MB per image
            cur = self.slots[slot] = aligned_scratch(nbytes, self.device) + (n,)
        return cur[1], cur[2]

    def tensor(self, slot=0):
        """the uint8 tensor that owns the slot's memory (its first 256-byte-aligned address is the workspace pointer)"""
        return self.slots[slot][0]


def open_device(device):
    """(torch, library, device index) for a handle on `device` (None: the current torch device); raises without a GPU"""
    import torch
    if not torch.cuda.is_available():
        raise _abi.AlinkError("no ROCm device visible: a-link_amd computes only on the GPU (no CPU fallback)")
    index = _abi.resolve_device(device)
    return torch, _abi.init(index), index


class Handle(object):
    """Owner of one C handle `self.h` of the `prefix` family (<prefix>_create / <prefix>_destroy)."""
    prefix = None
    h = None

    def _open(self, device):
        self.torch, self.lib, index = open_device(device)
        return index

    def _fn(self, name):
        return getattr(self.lib, self.prefix + "_" + name)

    def _create(self, index, *args):
        with _abi.on_device(index):                   # the handle lives on the device current at create
            self.h = self._fn("create")(*args) or None
        if not self.h:
            raise _abi.AlinkError(self.prefix + "_create: " + self.lib.alink_last_error().decode())

    def _destroy(self):
        if self.h:
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:                             # interpreter exit: the library may be gone already
            pass


class ImageNet(Handle):
    """An image network: `h`, `dtype`, `device` (int), `image_size`, `max_batch`, `grad_enabled`, and its `embed_device`."""
    lazy_range_check = False
    _cached = None                                    # what the last embed_with_cache kept for input_gradient: (n, ...)

    def _create(self, index, *args):
        Handle._create(self, index, *args)
        # the per-call entry points, bound once (VGG-16 has no range flag and no gradient pass); the workspace cache holds
        # the handle's value, not `self`: no reference cycle keeps a network and its device memory alive
        self._range_flag = getattr(self.lib, self.prefix + "_range_flag", None)
        h, fwd, grad = self.h, self._fn("workspace_bytes"), getattr(self.lib, self.prefix + "_grad_workspace_bytes", None)
        self.ws = Workspace(lambda n, slot: (grad if slot == "grad" else fwd)(h, n), self.torch.device("cuda", index))

    def load_tensors(self, params, subject):
        """every tensor the handle expects, from the dict `params`; then finalize (subject: "checkpoint is" | "weights are")"""
        info, load = self._fn("tensor_info"), self._fn("load")
        name, cnt = C.c_char_p(), C.c_size_t()
        for i in range(self._fn("num_tensors")(self.h)):
            _abi.check(info(self.h, i, C.byref(name), C.byref(cnt)))
            key = name.value.decode()
            if key not in params:
                raise KeyError("%s missing tensor %s" % (subject, key))
            a = np.ascontiguousarray(params[key], dtype=np.float32)
            _abi.check(load(self.h, name.value, _abi.ptr(a), a.size), "load " + key)
        _abi.check(self._fn("finalize")(self.h), self.prefix + "_finalize")

    def probe_images(self):
        """the three images scales and ranges are probed on at build time: uniform noise (seed 0), all 0, all 255"""
        torch = self.torch
        h, w = self.image_size
        g = torch.Generator(device="cpu").manual_seed(0)
        return torch.stack([torch.randint(0, 256, (h, w, 3), generator=g).float(), torch.zeros(h, w, 3),
                            torch.full((h, w, 3), 255.0)]).to("cuda:%d" % self.device)

    def _check_input(self, x):
        if x.ndim != 4 or tuple(x.shape[1:]) != self.image_size + (3,):
            raise ValueError("expected images of shape (N,%d,%d,3), got %s" % (self.image_size + (tuple(x.shape),)))

    # -- calibration (dtype 'f16x2') -------------------------------------------------------------------
    def _calibrate_chunks(self, x, merge, run, dtype=None):
        """run(chunk, n, ws, wsb, merge, stream) on every max_batch images of x: the first chunk sets the scales unless
        merge, every further chunk only lowers them"""
        if self.dtype != "f16x2":
            raise _abi.AlinkError("only dtype='f16x2' is calibrated")
        for i in range(0, x.shape[0], self.max_batch):
            xc = x[i:i + self.max_batch].to("cuda:%d" % self.device, dtype).contiguous()
            ws, wsb = self.ws.get(xc.shape[0])
            self.torch.cuda.synchronize(self.device)
            _abi.check(run(xc, xc.shape[0], ws, wsb, 1 if (merge or i) else 0, _abi.current_stream(self.device)),
                       self.prefix + "_calibrate")

    def _identity(self):
        """the fields (lists of ints) a calibration state must share with this network besides dtype"""
        raise NotImplementedError

    def _misfit(self, st):
        return "calibration state does not fit this network"

    def state(self):
        """The calibration state of the split-precision mode as a small dict of plain ints ({} for any other dtype): what
        has to travel with a checkpoint, and from the rank that calibrated to every other rank, for embeddings to be
        bit-identical there (include/alink_hip.h: alink_backbone_get_scales)."""
        n = self._fn("num_scales")(self.h)
        if n == 0:
            return {}
        e = (C.c_int * n)()
        _abi.check(self._fn("get_scales")(self.h, e, n), self.prefix + "_get_scales")
        return dict({"dtype": self.dtype}, **self._identity(), scale_exponents=[int(v) for v in e])

    def load_state(self, st):
        """Install scales saved by state() (same architecture and image size)."""
        if not st:
            return
        if st.get("dtype") != self.dtype or any(list(st.get(k, [])) != v for k, v in self._identity().items()):
            raise _abi.AlinkError(self._misfit(st))
        v = [int(x) for x in st["scale_exponents"]]
        _abi.check(self._fn("set_scales")(self.h, (C.c_int * len(v))(*v), len(v)), self.prefix + "_set_scales")

    # -- the float16 range ------------------------------------------------------------------------------
    def range_left(self, reset=True):
        """True if, since the last reset, some embedding came out non-finite (float16 storage has 5 exponent bits).  The
        flag is one word of pinned host memory that the last kernel of a forward writes: synchronise first."""
        return bool(self._range_flag(self.h, 1 if reset else 0))

    def check_range(self):
        """Synchronise this device and raise if a float16-storage forward left the range since the last check."""
        if self.dtype in F16_STORAGE:
            self.torch.cuda.synchronize(self.device)
            if self.range_left():
                raise _abi.AlinkError(RANGE_TEXT)

    def _checked(self, out, redo=None, mode=()):
        """float16 storage: a network whose activations leave +-65504 (deep nets with synthetic weights do) comes out as
        NaN.  Fail loudly instead of returning it (bf16 has the range).  The test is a flag the last kernel raises, read
        after ONE synchronisation per call — or, with lazy_range_check, only in check_range() and at the start of the next
        call.  Split precision re-calibrates on the offending batch `redo` (scales only go down) and re-runs once
        (`mode`: the positional arguments calibrate and embed_device take after the images); plain f16 raises."""
        if self.dtype not in F16_STORAGE or self.lazy_range_check:
            return out
        self.torch.cuda.synchronize(self.device)
        if self.range_left():
            if self.dtype == "f16x2" and redo is not None:
                self.calibrate(redo, *mode, merge=True)
                return self.embed_device(redo, *mode, out=out, _retry=False)
            raise _abi.AlinkError(RANGE_TEXT)
        return out

    # -- input gradient (FGSM / PGD extension) ----------------------------------------------------------
    def _cache_args(self, x, width):
        """the argument checks of embed_with_cache: (what _check_input returns, contiguous x, n, out, ws, wsb)"""
        if not self.grad_enabled:
            raise _abi.AlinkError("%s was built without enable_grad=True" % type(self).__name__)
        key = self._check_input(x)
        if x.dtype != self.torch.float32:
            raise ValueError("gradients need float32 pixels")
        x = x.contiguous()
        n = x.shape[0]
        assert 0 < n <= self.max_batch
        return (key, x, n, self.torch.empty((n, width), dtype=self.torch.float32, device=x.device)) + self.ws.get(n, "grad")

    def _grad_args(self, d, width):
        """the argument checks of input_gradient: (what embed_with_cache kept, float32 contiguous d, ws, wsb)"""
        if self._cached is None:
            raise _abi.AlinkError("input_gradient before embed_with_cache")
        d = d.to(self.torch.float32).contiguous()
        assert tuple(d.shape) == (self._cached[0], width)
        return (self._cached, d) + self.ws.get(self._cached[0], "grad")
