"""CPU: the two entry points of the few-pixel attack on the SmallRes student — alink_perturb_resize_multi (perturb + split + resize
in one pass) and alink_smallres_score_pairs (pair scores whose bits do not depend on the batch) — are exported by the built
library, declared in include/alink_hip.h and bound in _abi.py with the header's argument counts; the Python surface and the
driver's three search options exist."""
import os
import re

import a_link_amd  # noqa: F401
from a_link_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"alink_perturb_resize_multi": 12, "alink_smallres_score_pairs": 7}


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
    from a_link_amd import attack, siamese, smallres
    assert callable(getattr(smallres.SmallResNet, "score_pairs"))
    assert siamese.SmallRes._preprocess_is_prescale is True
    assert callable(attack._PixelScorer) and callable(attack._FeatureScorer)


def test_driver_knows_the_search_options_with_the_reference_defaults():
    from a_link_amd import ALINK_MTP, alink_loop
    p = ALINK_MTP.build_parser()
    f = p.parse_args([])
    assert (f.attack_pixels, f.attack_maxiter, f.attack_popsize) == (40, 50, 250)          # code/attack.py:91
    f = p.parse_args(["--attack_pixels", "3", "--attack_maxiter", "2", "--attack_popsize", "15"])
    assert (f.attack_pixels, f.attack_maxiter, f.attack_popsize) == (3, 2, 15)
    assert not hasattr(alink_loop.Flags, "attack_pixels")                                  # options of this driver only
