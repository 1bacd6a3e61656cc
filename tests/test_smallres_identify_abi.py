"""CPU: the four entry points of SmallRes gallery identification — alink_smallres_features (the tower, an image at a time),
alink_head_forward_rect / alink_smallres_score_features (the rectangular score matrix of two feature matrices) and
alink_identify_rows (each probe's argmax / rank on the device) — are exported by the built library, declared in
include/alink_hip.h and bound in _abi.py with the header's argument counts; the Python surface and the driver's --gallery_eval
exist, `Flags` is unchanged, and the host-only identification_stats is right on hand-made arrays."""
import os
import re

import numpy as np
import pytest

import a_link_amd  # noqa: F401
from a_link_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"alink_smallres_features": 6, "alink_head_forward_rect": 8, "alink_smallres_score_features": 8, "alink_identify_rows": 10}


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


def test_header_states_the_rect_limit():
    src = open(os.path.join(ROOT, "include", "alink_hip.h")).read()
    m = re.search(r"#define\s+ALINK_HEAD_RECT_MAX_SCORES\s+\(1ll\s*<<\s*(\d+)\)", src)
    assert m is not None and int(m.group(1)) == 28


def test_python_surface_exists():
    from a_link_amd import alink_loop, siamese, smallres
    for name in ("features", "score_matrix"):
        assert callable(getattr(smallres.SmallResNet, name))
    assert callable(smallres.identify_rows)
    assert callable(siamese.SmallRes.identify)
    assert callable(alink_loop.top1_identification_gallery) and callable(alink_loop.identification_stats)
    for fn in (siamese.SmallRes.identify, alink_loop.identification_stats, smallres.SmallResNet.features, smallres.SmallResNet.score_matrix):
        assert "EXTENSION" in fn.__doc__


def test_driver_knows_gallery_eval_and_flags_are_unchanged():
    from a_link_amd import ALINK_MTP, alink_loop
    p = ALINK_MTP.build_parser()
    assert p.parse_args([]).gallery_eval is False                                          # off unless asked for
    assert p.parse_args(["--gallery_eval"]).gallery_eval is True
    assert not hasattr(alink_loop.Flags, "gallery_eval")                                   # an option of this driver only
    flags = sorted(n for n in vars(alink_loop.Flags) if not n.startswith("_"))
    assert flags == sorted(["out_model", "ensemble_basepath", "disguised_basemodel", "noise", "ft_epochs", "batch_size", "dig_epochs",
                            "undig_epochs", "batch_send", "mixture_ratio", "alink_bs", "num_ensemble_models", "active_ratio",
                            "split_ratio", "disparity_ratio", "eps", "augment", "refine_models", "train_disguised_model",
                            "blind_strategy", "screen_settle", "settle_options"])


def test_identification_stats_on_hand_made_arrays():
    from a_link_amd.alink_loop import identification_stats
    #           probe:   0  1  2  3  4   5
    true = np.array([0, 1, 2, 3, 9, -1])                 # 9 and -1: persons that are not in a gallery of 4
    best = np.array([0, 2, 2, 0, 1, 3])                  # probes 0 and 2 find their own face first
    rank = np.array([0, 1, 0, 3, -1, -1])                # own face at place 0, 1, 0, 3; not ranked twice
    st = identification_stats(best, rank, true, ks=(1, 2, 4))
    assert st["rank1"] == 2 / 6.0
    assert st["cmc"] == {1: 2 / 6.0, 2: 3 / 6.0, 4: 4 / 6.0}
    assert st["cmc"][1] == st["rank1"]
    assert identification_stats([1], [0], [1])["cmc"] == {1: 1.0, 5: 1.0, 10: 1.0}         # the default ks
    assert identification_stats([], [], [], ks=(1,)) == {"rank1": 0.0, "cmc": {1: 0.0}}
    with pytest.raises(ValueError):
        identification_stats([0, 1], [0], [0, 1])
