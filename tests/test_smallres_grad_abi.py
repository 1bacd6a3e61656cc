"""CPU: the two entry points of the SmallRes pixel attack — alink_smallres_input_grad (the gradient of the loss with respect to
the pixels) and alink_resize_bilinear_grad (the adjoint of the bilinear resize) — are exported by the built library, declared in
include/alink_hip.h and bound in _abi.py with the header's argument counts."""
import os
import re

import a_link_amd  # noqa: F401
from a_link_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"alink_smallres_input_grad": 12, "alink_resize_bilinear_grad": 9}


def _declaration(name):
    src = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    return None if m is None else [a.strip() for a in m.group(1).split(",")]


def test_new_symbols_exported_declared_and_bound():
    lib = _abi.load()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), "library does not export %s" % name
        args = _declaration(name)
        assert args is not None, "include/alink_hip.h does not declare %s" % name
        assert len(args) == nargs, (name, args)
        assert name in _abi.PROTOTYPES, "_abi.py has no prototype for %s" % name
        res, argtypes = _abi.PROTOTYPES[name]
        assert res is _abi._i and len(argtypes) == nargs, (name, argtypes)


def test_python_surface_exists():
    from a_link_amd import noise, siamese, smallres
    assert callable(getattr(smallres.SmallResNet, "input_gradients"))
    assert callable(getattr(siamese.SmallRes, "input_gradients"))
    assert callable(noise.resize_images_grad)
