"""GPU: the checkpoint-tensor contract of the three image networks (csrc/net_host.h, TensorTable behind
alink_backbone_* / alink_resnet50_* / alink_vgg16_* num_tensors, tensor_info, load and finalize's "never loaded" check).
Nothing is finalized and no kernel is launched: each network at its smallest configuration, handles only."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, ENOTFOUND = -1, -4, -5      # include/alink_hip.h


def _create_ir(abi, lib):
    cfg = abi.IRCfg()
    cfg.units[:] = [1, 1, 1, 1]
    cfg.widths[:] = [64, 64, 128, 256, 512]
    cfg.height, cfg.width, cfg.emb, cfg.dtype, cfg.bn_eps = 112, 112, 512, abi.DT_BF16, 2e-5
    return lib.alink_backbone_create(C.byref(cfg))


NETS = {
    # name: (entry-point prefix, create, the network as the "not part of" message calls it)
    "ir": ("alink_backbone", _create_ir, "the configured network"),
    "resnet50": ("alink_resnet50", lambda abi, lib: lib.alink_resnet50_create(224, 224, abi.DT_BF16, 1e-3), "the VGGFace2 ResNet-50"),
    "vgg16": ("alink_vgg16", lambda abi, lib: lib.alink_vgg16_create(32, 32, abi.DT_BF16), "the VGGFace VGG-16"),
}


def _fails(abi, rc, code, *needles):
    """rc is `code`, and the error the bindings raise for it carries every needle."""
    assert rc == code, (rc, abi.load().alink_last_error())
    with pytest.raises(abi.AlinkError) as e:
        abi.check(rc, "call")
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


@pytest.mark.parametrize("net", sorted(NETS))
def test_tensor_table_contract(gpu, net):
    prefix, create, what = NETS[net]
    lib = gpu.load()
    fn = lambda name: getattr(lib, prefix + "_" + name)
    h = create(gpu, lib)
    assert h, lib.alink_last_error()
    try:
        def table():
            name, cnt = C.c_char_p(), C.c_size_t()
            rows = []
            for i in range(fn("num_tensors")(h)):
                gpu.check(fn("tensor_info")(h, i, C.byref(name), C.byref(cnt)), "tensor_info")
                rows.append((name.value, int(cnt.value)))
            return rows

        # tensor_info enumerates num_tensors names, the same ones in the same order every time, each with a positive count
        rows = table()
        assert len(rows) == fn("num_tensors")(h) > 4
        assert rows == table()
        assert len({n for n, _ in rows}) == len(rows)
        assert all(n and c > 0 for n, c in rows)
        name, cnt = C.c_char_p(), C.c_size_t()
        _fails(gpu, fn("tensor_info")(h, len(rows), C.byref(name), C.byref(cnt)), EINVAL, "tensor index out of range")
        _fails(gpu, fn("tensor_info")(h, -1, C.byref(name), C.byref(cnt)), EINVAL, "tensor index out of range")

        # load: an unknown name, a wrong count, NULL name, NULL data
        n0, c0 = rows[0]
        buf = np.zeros(c0 + 1, np.float32)
        _fails(gpu, fn("load")(h, b"no_such_tensor", gpu.ptr(buf), c0), ENOTFOUND, "tensor no_such_tensor is not part of " + what)
        _fails(gpu, fn("load")(h, n0, gpu.ptr(buf), c0 + 1), EINVAL, "tensor %s:" % n0.decode(), "expected %d elements" % c0,
               "got %d" % (c0 + 1))
        _fails(gpu, fn("load")(h, None, gpu.ptr(buf), c0), EINVAL, "NULL argument")
        _fails(gpu, fn("load")(h, n0, None, c0), EINVAL, "NULL argument")

        # finalize with tensors missing names the first one in table order; it fails before anything is built
        first, later = 3, len(rows) - 1
        zeros = np.zeros(max(c for _, c in rows), np.float32)
        for i, (n, c) in enumerate(rows):
            if i not in (first, later):
                gpu.check(fn("load")(h, n, gpu.ptr(zeros), c), "load")
        _fails(gpu, fn("finalize")(h), ESTATE, "tensor %s was never loaded" % rows[first][0].decode())
        # ... and the handle still takes the tensor (it was not finalized)
        gpu.check(fn("load")(h, rows[first][0], gpu.ptr(zeros), rows[first][1]), "load")
        _fails(gpu, fn("finalize")(h), ESTATE, "tensor %s was never loaded" % rows[later][0].decode())
    finally:
        fn("destroy")(h)
