"""The feature-map gradient's entry points without a GPU: declared in the header, bound in _lib, and no CPU path behind the ops."""
import os
import re

import pytest
import torch

from mgnns_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mgnns_map_argmax", "mgnns_imgbank_dgrad")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "mgnns_hip.h")).read()
    declared = set(re.findall(r"\b(mgnns_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW:
        assert name in declared, "%s is not declared in include/mgnns_hip.h" % name
        assert name in _lib.SIGNATURES
        assert hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(_lib.SIGNATURES[name])
    assert int(re.search(r"#define MGNNS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 23


def test_the_ops_refuse_cpu_tensors():
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.map_argmax(torch.zeros(2, 16, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.imgbank_dgrad(torch.zeros(2, 4, 8), torch.zeros(8, 16))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.imgbank_dgrad(None, torch.zeros(8, 16), torch.zeros(2, 16), torch.zeros(2, 16, dtype=torch.int32), positions=4)
