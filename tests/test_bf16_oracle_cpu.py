"""oracle/bf16_path.py, the bf16-mode emulation the GPU tests hold the kernels to (tests/test_bf16_path_gpu.py): its rounding
helper is torch's bf16 cast, with every rounding point off it is restatement.forward, and every rounding point it has is live."""
import numpy as np
import pytest
import torch

from mgnns_amd import synth
from mgnns_amd.harness import build_model
from oracle import bf16_path as E
from oracle import restatement as R
from tests import helpers as H


def test_rounding_helper_is_torch_bf16_cast_bit_for_bit():
    rs = np.random.RandomState(0)
    vals = [rs.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rs.randint(-30, 30, 20000).astype(np.float32)]
    # exact ties between two bf16 neighbours (low half 0x8000) with an even and an odd upper half, either sign
    hi = rs.randint(0, 0x7F7F, 4000).astype(np.uint32)
    ties = (hi << 16) | 0x8000
    vals.append(np.concatenate([ties, ties | 0x80000000, ties + 0x7FFF, ties + 1]).astype(np.uint32).view(np.float32))
    special = np.array([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x80000001, 0x807FFFFF,   # subnormals
                        0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF, 0xFF7F8000, 0xFF7FFFFF,                          # near bf16 max
                        0x7F800000, 0xFF800000, 0x00000000, 0x80000000,                                      # +-inf, +-0
                        0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7F8000FF], dtype=np.uint32)        # NaN
    vals.append(special.view(np.float32))
    x = np.concatenate(vals)
    mine = E.bf16_bits(x)
    ref = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(x)
    assert np.array_equal(mine[~nan], ref[~nan])
    as_f = lambda b: (b.astype(np.uint32) << 16).view(np.float32)
    assert nan.sum() == 5 and np.isnan(as_f(mine[nan])).all() and np.isnan(as_f(ref[nan])).all()
    t = torch.from_numpy(x[~nan]).double()
    assert torch.equal(E.bf16_round(t), t.float().to(torch.bfloat16).double())


def _setup(cfg_name, B):
    g = H.load_golden("full_%s.npz" % cfg_name)
    adj = H.load_golden("adjacency.npz")
    cfg = synth.CONFIGS[cfg_name]
    pmi, count = synth.synth_pmi(cfg.V, seed=cfg.seed + 17)
    model = build_model(cfg, pmi, count, adj["object_t04_A"], adj["place_t03_A"], g["label_query"])
    p = {k: v.detach() for k, v in model.state_dict().items()}
    inp = synth.make_inputs(cfg, B=int(g["B"]), pmi=pmi)
    sub = {k: torch.as_tensor(v[:B] if k != "label_query" else v) for k, v in inp.items()}
    return cfg, g, p, pmi, sub


@pytest.mark.parametrize("attention", ["faithful", "folded"])
@pytest.mark.parametrize("cfg_name", ["mvsa_single_b8", "tumemo_b64"])
def test_no_rounding_is_the_restatement(cfg_name, attention):
    """With every rounding point off the emulation is restatement.forward.  restatement.forward cannot run in fp64 (it casts the
    label query to fp32, runs torch's fp32 nn.LSTM and the float32 numpy text GCN), so the gate is fp32 summation order: 3e-6 of
    the logits' scale (measured 1.1e-6 / 5.5e-7); the reference's own golden logits agree to the same level."""
    cfg, g, p, pmi, sub = _setup(cfg_name, 8)
    lq = torch.from_numpy(g["label_query"])
    ref, rparts = R.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram, label_query=lq, return_parts=True)
    got, parts = E.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram, label_query=lq, attention=attention,
                           rounding=(), return_parts=True)
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert H.relerr(got, ref) < 3e-6
    assert H.relerr(got, g["logits"][:8]) < 3e-6
    for k in ("text_bank", "bank_object", "bank_place", "tio", "tip", "iot", "ipt"):
        assert H.relerr(parts[k], rparts[k]) < 3e-6, k
    assert torch.equal(parts["text_bank"], parts["text_bank_bf16"])
    rounded = E.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram, label_query=lq, attention=attention)
    assert 1e-3 < H.maxabs(rounded, ref) < 2e-2            # the bf16 network's distance from the fp32 one (bf16 noise)


@pytest.mark.parametrize("attention", ["faithful", "folded"])
def test_every_rounding_point_is_live(attention):
    """Switching on any single rounding point moves the logits: none is dead code.  mvsa_single_b8 has one layer per stack, so the
    next-layer query (tail_q) is checked on the first four samples of tumemo_b64 (two layers)."""
    live = [pt for pt in E.POINTS if pt not in (E.FOLDED_ONLY if attention == "faithful" else E.FAITHFUL_ONLY)]
    for cfg_name, points in (("mvsa_single_b8", [pt for pt in live if pt != "tail_q"]), ("tumemo_b64", ["tail_q"])):
        cfg, g, p, pmi, sub = _setup(cfg_name, 8 if cfg_name == "mvsa_single_b8" else 4)
        run = lambda rounding: E.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram,
                                         label_query=torch.from_numpy(g["label_query"]), attention=attention, rounding=rounding)
        base = run(())
        for pt in points:
            d = H.maxabs(run((pt,)), base)
            assert d > 1e-7, (cfg_name, pt, d)
    # the points of the other attention form change nothing
    cfg, g, p, pmi, sub = _setup("mvsa_single_b8", 2)
    dead = E.FOLDED_ONLY if attention == "faithful" else E.FAITHFUL_ONLY
    run = lambda rounding: E.forward(p, sub, pmi, cfg.n_head, cfg.d_kv, cfg.stack_num, cfg.ngram,
                                     label_query=torch.from_numpy(g["label_query"]), attention=attention, rounding=rounding)
    assert torch.equal(run(dead), run(()))


def test_unknown_rounding_point_is_refused():
    with pytest.raises(ValueError, match="unknown rounding"):
        E.img_bank(torch.zeros(1, 64, 16), torch.zeros(8, 64), torch.zeros(8), rounding=("imgbank_xx",))


def test_label_tail_emulation_terms3_is_the_restatement():
    """label_tail(terms=3) (split-bf16, fp32-class) is restatement's label attention + tail; terms=1 is bf16 noise away."""
    g = H.load_golden("label_attention.npz")
    pc = H.params_for(H.label_attention_shapes("object", 80))
    lq = torch.from_numpy(g["label_query"])
    Q = torch.nn.functional.linear(lq, pc["object_attention.w_q.weight"], pc["object_attention.w_q.bias"])
    rs = np.random.RandomState(81)
    G = torch.from_numpy((0.05 * rs.standard_normal((80, 2048))).astype(np.float32))
    pooled = torch.from_numpy(np.maximum(rs.standard_normal((5, 2048)), 0).astype(np.float32))
    ref = R.label_attention_tail(pc, "object", R.label_attention(pc, "object_attention", lq, pooled @ G.t()))
    got3, _ = E.label_tail(pc, "object", pooled, G, Q, 5, terms=3)
    got1, _ = E.label_tail(pc, "object", pooled, G, Q, 5, terms=1)
    assert H.relerr(got3, ref) < 3e-6
    assert 1e-4 < H.relerr(got1, ref) < 2e-2
