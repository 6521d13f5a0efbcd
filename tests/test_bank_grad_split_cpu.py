"""The training bank-precision switch and the split-bf16 gradient entry points without a GPU: the setter's surface, the header
against the binding, and the refusals that do not change."""
import os
import re

import pytest
import torch

from mgnns_amd import _lib, harness, synth
from mgnns_amd.model import Multi_GCN_Multihead_Att

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mgnns_imgbank_wgrad_split", "mgnns_imgbank_dgrad_split")
NEW_SIZES = ("mgnns_imgbank_wgrad_split_workspace_bytes", "mgnns_imgbank_dgrad_split_workspace_bytes")


def cpu_model(name="mvsa_single_b8", **opt_extra):
    cfg = synth.CONFIGS[name]
    pmi, count = synth.synth_pmi(cfg.V, seed=2)
    inp = synth.make_inputs(cfg, B=2, seed=7, pmi=pmi)
    if not opt_extra:
        A_obj, A_place = harness.synthetic_adjacencies(cfg)
        return harness.build_model(cfg, pmi, count, A_obj, A_place, inp["label_query"])
    tm = harness.Text_model_from_parts(harness.make_vocab(cfg.V), pmi, count, cfg.NL, cfg.ngram, 0.5)
    return Multi_GCN_Multihead_Att(dict(cfg.opt(), **opt_extra), cfg.NL, tm, None, None, cfg.C_obj, cfg.C_place,
                                   label_glove=torch.as_tensor(inp["label_query"]))


def test_the_setter():
    model = cpu_model("tumemo_b64")
    assert model.train_bank_precision == 'fp32'
    keys = set(model.state_dict())
    assert model.set_train_bank_precision('bf16x3') is model and model.train_bank_precision == 'bf16x3'
    assert model.set_train_bank_precision('fp32') is model and model.train_bank_precision == 'fp32'
    for bad in ('bf16', 'fp16', None, 3):
        with pytest.raises(ValueError, match="train_bank_precision"):
            model.set_train_bank_precision(bad)
    assert model.train_bank_precision == 'fp32'
    assert set(model.state_dict()) == keys and len(keys) == 249


def test_the_option_is_honoured():
    assert cpu_model(train_bank_precision='bf16x3').train_bank_precision == 'bf16x3'
    with pytest.raises(ValueError, match="train_bank_precision"):
        cpu_model(train_bank_precision='bf16')


def test_header_and_binding_agree_on_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mgnns_hip.h")).read()
    declared = set(re.findall(r"\b(mgnns_[a-z0-9_]+)\s*\(", hdr))
    assert int(re.search(r"#define MGNNS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION >= 25
    for name in NEW:
        assert name in declared, "%s is not declared in include/mgnns_hip.h" % name
        assert name in _lib.SIGNATURES
    for name in NEW_SIZES:
        assert name in declared, "%s is not declared in include/mgnns_hip.h" % name
        assert name in _lib.SIZE_GETTERS and len(_lib.SIZE_GETTERS[name]) == 4
    assert len(_lib.SIGNATURES["mgnns_imgbank_wgrad_split"]) == len(_lib.SIGNATURES["mgnns_imgbank_wgrad"])
    assert len(_lib.SIGNATURES["mgnns_imgbank_dgrad_split"]) == len(_lib.SIGNATURES["mgnns_imgbank_dgrad"]) + 2
    L = _lib.lib()
    for name in NEW + NEW_SIZES:
        assert hasattr(L, name)
    assert L.mgnns_imgbank_dgrad_split_workspace_bytes(0, 16, 4, 8) == 64 == L.mgnns_imgbank_wgrad_split_workspace_bytes(0, 16, 4, 8)


def test_training_in_a_bf16_precision_is_still_refused():
    model = cpu_model().train().freeze_text_encoders()
    model.set_train_bank_precision('bf16x3')
    model._refuse_untrainable()
    for prec in ('bf16', 'bf16x3'):
        model.set_precision(prec)
        with pytest.raises(NotImplementedError, match="fp32 only"):
            model._refuse_untrainable()
