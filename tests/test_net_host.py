"""Host test of a-link_amd/net_host.py — the plumbing IRBackbone, VGGResNet50, VGGFace16, DenseHead and SmallResNet share — on
the CPU, with no GPU and no library call: the library is a stub whose entry points are plain Python callables that record
their calls, and the three image networks are built by their own constructors on top of it."""
import contextlib
import ctypes as C
import types
import weakref

import numpy as np
import pytest
import torch

from a_link_amd import _abi, net_host
from a_link_amd.backbone import IRBackbone
from a_link_amd.resnet50 import VGGResNet50
from a_link_amd.vgg16 import VGGFace16

PREFIXES = ("alink_backbone", "alink_resnet50", "alink_vgg16")


class StubLib(object):
    """lib.<prefix>_<name>(*args) records (full name, args) and answers with the method _<name> below (0 if there is none)"""

    def __init__(self, tensors=(), exponents=(), flags=(), create=1):
        self.tensors = [(k.encode(), n) for k, n in tensors]       # (name, element count) in tensor_info order
        self.exponents, self.flags, self.handle = list(exponents), list(flags), create
        self.calls, self.loaded = [], []

    def __getattr__(self, name):
        short = next((name[len(p) + 1:] for p in PREFIXES if name.startswith(p + "_")), name)
        impl = getattr(type(self), "_" + short, None)

        def call(*args):
            self.calls.append((name, args))
            return impl(self, *args) if impl else 0
        return call

    def names(self, short=None):
        return [n for n, _ in self.calls if short is None or n.endswith("_" + short)]

    def _create(self, *args):
        return self.handle

    def _alink_last_error(self):
        return b"the stub has no memory"

    def _num_tensors(self, h):
        return len(self.tensors)

    def _tensor_info(self, h, i, name, count):
        name._obj.value, count._obj.value = self.tensors[i]
        return 0

    def _load(self, h, name, ptr, count):
        self.loaded.append((name, np.ctypeslib.as_array((C.c_float * count).from_address(ptr.value)).copy()))
        return 0

    def _workspace_bytes(self, h, n):
        return 1000 * n

    def _grad_workspace_bytes(self, h, n):
        return 5000 * n

    def _range_flag(self, h, reset):
        return self.flags.pop(0) if self.flags else 0

    def _num_scales(self, h):
        return len(self.exponents)

    def _get_scales(self, h, e, n):
        e[:] = self.exponents
        return 0

    def _set_scales(self, h, e, n):
        self.exponents = [e[i] for i in range(n)]
        return 0

    def _feature_size(self, h):
        return 25088


@pytest.fixture
def host(monkeypatch):
    """open_device and on_device without a GPU: host(lib) makes `lib` what the next handles are built on; host.syncs counts
    torch.cuda.synchronize calls"""
    box = types.SimpleNamespace(lib=None, syncs=[])
    fake = types.SimpleNamespace(cuda=types.SimpleNamespace(synchronize=box.syncs.append), device=lambda *a: torch.device("cpu"),
                                 float32=torch.float32, empty=torch.empty)
    monkeypatch.setattr(net_host, "open_device", lambda device: (fake, box.lib, 0))
    monkeypatch.setattr(_abi, "on_device", lambda device: contextlib.nullcontext())

    def use(lib):
        box.lib = lib
        return lib
    use.syncs = box.syncs
    return use


IR_PARAMS = dict({"stage%d_unit%d_conv1_weight" % (s, u): np.zeros(1, np.float32) for s, u in ((1, 1), (2, 1), (2, 2), (3, 1), (4, 1))},
                 fc1_weight=np.asfortranarray(np.arange(12, dtype=np.float64).reshape(3, 4)), conv0_weight=np.ones((2, 5)))
KERAS_PARAMS = {"conv1/kernel": np.asfortranarray(np.arange(12, dtype=np.float64).reshape(3, 4)), "conv1/bias": np.ones((2, 5))}
BUILD = {"alink_backbone": lambda **kw: IRBackbone(dict(IR_PARAMS, **kw.pop("more", {})), image_size=(32, 32), **kw),
         "alink_resnet50": lambda **kw: VGGResNet50(image_size=(224, 224), weights=dict(KERAS_PARAMS, **kw.pop("more", {})), **kw),
         "alink_vgg16": lambda **kw: VGGFace16(image_size=(224, 224), weights=dict(KERAS_PARAMS, **kw.pop("more", {})), **kw)}
LISTED = {"alink_backbone": [("fc1_weight", 12), ("conv0_weight", 10)], "alink_resnet50": [("conv1/kernel", 12), ("conv1/bias", 10)],
          "alink_vgg16": [("conv1/kernel", 12), ("conv1/bias", 10)]}


# ---- aligned scratch and the workspace cache ------------------------------------------------------------------------------------
def _inside(t, p, usable):
    return t.data_ptr() <= p and p + usable <= t.data_ptr() + t.numel()


def test_aligned_scratch():
    for nbytes in (0, 1, 255, 256, 1000):
        t, p, usable = net_host.aligned_scratch(nbytes, "cpu")
        assert t.dtype == torch.uint8 and p % 256 == 0 and usable >= nbytes and _inside(t, p, usable)


def test_workspace_cache_grows_only_and_drops_before_it_allocates(monkeypatch):
    asked = []
    ws = net_host.Workspace(lambda n, slot: asked.append((n, slot)) or 1000 * n, "cpu")
    for n in (5, 3, 5):
        p, usable = ws.get(n)
        assert p % 256 == 0 and usable >= 1000 * n and _inside(ws.tensor(), p, usable)
    assert asked == [(5, 0)]                                    # 5, 3, 5 images: one allocation
    # 3 then 5 images: two allocations, and the first tensor is gone when the second is asked for
    asked[:] = []
    ws = net_host.Workspace(lambda n, slot: asked.append((n, slot)) or 1000 * n, "cpu")
    ws.get(3)
    first = weakref.ref(ws.tensor())
    assert first() is not None
    real, seen = net_host.aligned_scratch, []

    def allocate(nbytes, device):
        seen.append(first() is None)
        return real(nbytes, device)
    monkeypatch.setattr(net_host, "aligned_scratch", allocate)
    p, usable = ws.get(5)
    assert asked == [(3, 0), (5, 0)] and seen == [True] and usable >= 5000 and _inside(ws.tensor(), p, usable)


def test_workspace_slots_are_independent():
    asked = []
    ws = net_host.Workspace(lambda n, slot: asked.append((n, slot)) or (5000 if slot == "grad" else 1000) * n, "cpu")
    got = {slot: ws.get(n, slot) for slot, n in ((0, 4), (1, 2), ("grad", 3))}
    assert asked == [(4, 0), (2, 1), (3, "grad")]
    assert len({ws.tensor(slot).data_ptr() for slot in got}) == 3 and got["grad"][1] >= 15000
    assert all(ws.get(n, slot) == got[slot] for slot, n in ((0, 4), (1, 1), ("grad", 3)))      # nothing moved, nothing asked
    assert len(asked) == 3
    ws.get(3, 1)                                                # slot 1 grows alone
    assert asked[3:] == [(3, 1)] and ws.get(4, 0) == got[0] and ws.get(3, "grad") == got["grad"]


# ---- load_tensors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", PREFIXES)
def test_load_tensors_walks_the_handle_s_list_and_finalizes_last(host, prefix):
    lib = host(StubLib(tensors=LISTED[prefix]))
    net = BUILD[prefix]()
    assert net.h == 1 and net.lib is lib
    # every listed tensor once, in tensor_info order, as contiguous float32 of the stated size (the dict holds a float64
    # Fortran-ordered array and a float64 C-ordered one: what reaches `load` is their C-order float32 flattening)
    assert [k for k, _ in lib.loaded] == [k.encode() for k, _ in LISTED[prefix]]
    assert [a[3] for n, a in lib.calls if n == prefix + "_load"] == [12, 10]
    assert np.array_equal(lib.loaded[0][1], np.arange(12, dtype=np.float32)) and lib.loaded[0][1].dtype == np.float32
    assert np.array_equal(lib.loaded[1][1], np.ones(10, np.float32))
    assert lib.names("finalize") == [prefix + "_finalize"]
    walk = [n for n in lib.names() if n.rsplit("_", 1)[-1] in ("info", "load", "finalize")]
    assert walk == [prefix + "_tensor_info", prefix + "_load"] * 2 + [prefix + "_finalize"]


@pytest.mark.parametrize("prefix,text", [("alink_backbone", "checkpoint is missing tensor bn9_gamma"),
                                         ("alink_resnet50", "weights are missing tensor bn9_gamma"),
                                         ("alink_vgg16", "weights are missing tensor bn9_gamma")])
def test_a_missing_tensor_is_named_and_nothing_is_finalized(host, prefix, text):
    lib = host(StubLib(tensors=LISTED[prefix][:1] + [("bn9_gamma", 4)] + LISTED[prefix][1:]))
    with pytest.raises(KeyError, match=text):
        BUILD[prefix]()
    assert len(lib.loaded) == 1 and lib.names("finalize") == []


# ---- state / load_state ---------------------------------------------------------------------------------------------------------
def _split_precision(host, prefix, exponents, **kw):
    """a handle in dtype 'f16x2' on the stub (built as bf16: the constructor of the split-precision mode calibrates on the device)"""
    lib = host(StubLib(tensors=LISTED[prefix], exponents=exponents))
    net = BUILD[prefix](**kw)
    net.dtype = "f16x2"
    return net, lib


@pytest.mark.parametrize("prefix", PREFIXES[:2])
def test_state_round_trip(host, prefix):
    a, la = _split_precision(host, prefix, [3, -2, 0, 17])
    st = a.state()
    want = {"dtype": "f16x2", "image_size": list(a.image_size), "scale_exponents": [3, -2, 0, 17]}
    if prefix == "alink_backbone":
        want["units"] = [1, 2, 1, 1]
    assert st == want and all(type(v) is int for v in st["scale_exponents"])
    b, lb = _split_precision(host, prefix, [0, 0, 0, 0])
    b.load_state(st)
    assert lb.exponents == [3, -2, 0, 17] and b.state() == st
    # {} is accepted and calls nothing; a handle without scales has the state {}
    before = len(lb.calls)
    b.load_state({})
    assert len(lb.calls) == before
    c, _ = _split_precision(host, prefix, [])
    assert c.state() == {}


@pytest.mark.parametrize("prefix", PREFIXES[:2])
def test_a_state_that_does_not_fit_is_refused_before_set_scales(host, prefix):
    a, _ = _split_precision(host, prefix, [1, 2, 3])
    st = a.state()
    b, lb = _split_precision(host, prefix, [0, 0, 0])
    wrong = [dict(st, dtype="f16"), dict(st, image_size=[64, 64])]
    if prefix == "alink_backbone":
        wrong.append(dict(st, units=[1, 1, 1, 1]))
    for bad in wrong:
        with pytest.raises(_abi.AlinkError, match="does not fit this"):
            b.load_state(bad)
    assert lb.names("set_scales") == [] and lb.exponents == [0, 0, 0]
    if prefix == "alink_backbone":                              # the backbone's text says what differs
        with pytest.raises(_abi.AlinkError, match=r"f16x2 \[1, 1, 1, 1\] network at \[32, 32\] does not fit this f16x2 \[1, 2, 1, 1\]"):
            b.load_state(wrong[2])


# ---- the float16 range rule -----------------------------------------------------------------------------------------------------
class _RangeNet(net_host.ImageNet):
    """ImageNet's rule around a forward that only counts: embed_device / calibrate with the signatures of VGGResNet50"""
    prefix = "alink_resnet50"

    def __init__(self, dtype):
        self.torch, self.lib, self.device = net_host.open_device(None)
        self.dtype, self.forwards, self.calibrated = dtype, 0, []
        self._create(self.device)

    def calibrate(self, x, preprocessed=False, merge=False):
        self.calibrated.append((x, preprocessed, merge))

    def embed_device(self, x, preprocessed=False, out=None, _retry=True):
        self.forwards += 1
        return self._checked(out if out is not None else ["features"], x if _retry else None, (preprocessed,))


def test_range_rule_split_precision_recalibrates_once_then_raises(host):
    lib = host(StubLib(flags=[1, 0]))
    net, batch = _RangeNet("f16x2"), object()
    out = net.embed_device(batch, True)
    assert out == ["features"] and net.forwards == 2 and net.calibrated == [(batch, True, True)]
    assert len(lib.names("range_flag")) == 2 and len(host.syncs) == 2
    lib.flags[:] = [1, 1]                                       # raised again after the re-calibration
    with pytest.raises(_abi.AlinkError, match="float16 range"):
        net.embed_device(batch)
    assert net.forwards == 4 and len(net.calibrated) == 2


def test_range_rule_plain_f16_raises_at_once_and_bf16_never_looks(host):
    lib = host(StubLib(flags=[1]))
    net = _RangeNet("f16")
    with pytest.raises(_abi.AlinkError, match="float16 range"):
        net.embed_device(object())
    assert net.forwards == 1 and net.calibrated == []
    net.check_range()                                           # the flag was cleared by the read
    lib = host(StubLib(flags=[1]))
    net = _RangeNet("bf16")
    del host.syncs[:]
    assert net.embed_device(object()) == ["features"] and net.forwards == 1
    net.check_range()
    assert lib.names("range_flag") == [] and host.syncs == []
    # lazy_range_check defers the read of a 16-bit mode to check_range
    lib = host(StubLib(flags=[1]))
    net = _RangeNet("f16")
    net.lazy_range_check = True
    assert net.embed_device(object()) == ["features"] and lib.names("range_flag") == []
    with pytest.raises(_abi.AlinkError, match="float16 range"):
        net.check_range()


# ---- the handle base ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefix", PREFIXES)
def test_destroy_runs_once(host, prefix):
    lib = host(StubLib(tensors=LISTED[prefix]))
    net = BUILD[prefix]()
    net.__del__()
    assert net.h is None
    net.__del__()
    del net
    assert lib.names("destroy") == [prefix + "_destroy"]


@pytest.mark.parametrize("prefix", PREFIXES)
def test_a_null_handle_raises_with_the_library_s_words(host, prefix):
    lib = host(StubLib(tensors=LISTED[prefix], create=None))
    with pytest.raises(_abi.AlinkError, match=prefix + "_create: the stub has no memory"):
        BUILD[prefix]()
    assert lib.names("destroy") == [] and lib.names("num_tensors") == []
