"""The cluster launches' scratch slots (ops._scratch_slot) on their normal grow path: a batch of one 16-sample tile, then one of
three tiles on the SAME pack and stream ("Derived packs and launch scratch")."""
import numpy as np
import pytest
import torch

from mgnns_amd import ops
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(x):
    return torch.as_tensor(x).to(DEV).contiguous()


def _label_tail_case():
    """ops.label_tail_bf16(terms=3) on the object channel of test_fused_label_tail_bf16_vs_oracle."""
    tag, C = "object", 80
    p = {k: v.to(DEV).contiguous() for k, v in H.params_for(H.label_attention_shapes(tag, C)).items()}
    a = tag + "_attention."
    Q = ops.linear(dev(H.load_golden("label_attention.npz")["label_query"]), p[a + "w_q.weight"], p[a + "w_q.bias"])
    wc = ops.matmul(p[tag + "_linear_5.weight"], p[a + "fc.weight"])
    bc = ops.linear(p[a + "fc.bias"][None, :].contiguous(), p[tag + "_linear_5.weight"], p[tag + "_linear_5.bias"])[0].contiguous()
    sp = lambda w: ops.pack_weight_bf16_split(w.contiguous())
    rs = np.random.RandomState(C + 1)
    Gp = sp(dev((0.05 * rs.standard_normal((C, 2048))).astype(np.float32)))
    nq = (sp(dev((0.05 * rs.standard_normal((1024, 300))).astype(np.float32))), dev((0.05 * rs.standard_normal(1024)).astype(np.float32)), 1024)
    halves = dev(np.maximum(rs.standard_normal((33, 2, 2048)), 0).astype(np.float32))

    def pack():
        return {"wk": sp(p[a + "w_k.weight"]), "bk": p[a + "w_k.bias"], "wv": sp(p[a + "w_v.weight"]), "bv": p[a + "w_v.bias"],
                "wc": sp(wc), "bc": bc, "n5": 100, "C": C, "xl": sp(p[tag + "_x_linear.weight"]), "bxl": p[tag + "_x_linear.bias"],
                "n_out": 300}

    def launch(packed, B):
        return ops.label_tail_bf16(halves[:B].contiguous(), Gp, Q, 5, packed, next_q=nq, terms=3)
    return "_cluster_ws", pack, launch


def _mha_tail_bf16_case():
    """ops.mha_tail_bf16(terms=1, ksplit=True) on the four-head layer of test_mha_tail_bf16_k_split_over_the_cluster."""
    Hn, name = 4, "h4_img"
    p = {k: v.to(DEV).contiguous() for k, v in H.params_for(H.mha_shapes(Hn), prefix=name + ".").items()}
    a, f = name + ".slf_attn.", name + ".pos_ffn."
    w1 = p[f + "w_1.weight"].squeeze(-1).contiguous()
    w2 = p[f + "w_2.weight"].squeeze(-1).contiguous()
    nx = (ops.pack_weight_bf16_split(p[a + "w_qs.weight"]), p[a + "w_qs.bias"], Hn * 128)
    rs = np.random.RandomState(Hn)
    o = dev(rs.standard_normal((33, Hn * 128)).astype(np.float32))
    q = dev(rs.standard_normal((33, 300)).astype(np.float32))

    def pack():
        return {"fc_b": p[a + "fc.bias"], "g1": p[a + "layer_norm.gamma"], "be1": p[a + "layer_norm.beta"], "b1": p[f + "w_1.bias"],
                "b2": p[f + "w_2.bias"], "g2": p[f + "layer_norm.gamma"], "be2": p[f + "layer_norm.beta"],
                "fc": ops.pack_weight_bf16_split(p[a + "fc.weight"]), "w1": ops.pack_weight_bf16_split(w1),
                "w2": ops.pack_weight_bf16_split(w2)}

    def launch(packed, B):
        return ops.mha_tail_bf16(o[:B].contiguous(), q[:B].contiguous(), packed, 1e-6, nx, terms=1, ksplit=True)
    return "_cluster_ws_ks", pack, launch


def _mha_tail_c16_case():
    """ops.mha_tail_c16(ksplit=True) on the four-head operands of test_mha_tail_c16_cluster_forms_agree_and_match_fp64."""
    Hn = 4
    g = torch.Generator(device=DEV).manual_seed(11 + Hn)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g) * 0.05
    HD = Hn * 300
    ldc = (HD + 31) // 32 * 32
    c = torch.zeros(33, ldc, device=DEV, dtype=torch.bfloat16)
    c[:, :HD] = torch.randn(33, HD, device=DEV, generator=g).to(torch.bfloat16)
    q = torch.randn(33, 300, device=DEV, generator=g)
    fc, w1, w2, wq = r(300, HD), r(300, 300), r(300, 300), r(HD, 300)
    small = {"fc_b": r(300), "g1": r(300) + 1, "be1": r(300), "b1": r(300), "b2": r(300), "g2": r(300) + 1, "be2": r(300)}
    nx = (ops.pack_weight_bf16_split(wq), r(HD), HD)

    def pack():
        return dict(small, fc=ops.pack_weight_bf16_split(fc), w1=ops.pack_weight_bf16_split(w1), w2=ops.pack_weight_bf16_split(w2))

    def launch(packed, B):
        return ops.mha_tail_c16(c[:B].contiguous(), q[:B].contiguous(), packed, 1e-6, nx, ksplit=True)
    return "_cluster_ws", pack, launch


@pytest.mark.parametrize("case", [_label_tail_case, _mha_tail_bf16_case, _mha_tail_c16_case])
def test_cluster_scratch_grows_from_one_tile_to_three_on_the_same_pack(case):
    """B = 16 (one tile), then B = 33 (three tiles) on one pack and stream: the result is the one a freshly built pack gives, bit
    for bit; the one-tile buffer is kept in packed["_retired"] (a captured graph may hold its address); the slot dict holds one entry,
    under the current scratch key, with its counters back at zero; and B = 16 again neither shrinks nor reallocates."""
    name, pack, launch = case()
    packed = pack()
    key = ops._scratch_key()
    launch(packed, 16)
    one = packed[name][key]
    assert one[0] == 1 and "_retired" not in packed
    got = launch(packed, 33)
    three = packed[name][key]
    assert three is not one and three[0] == 3 and one[0] == 1
    assert len(packed["_retired"]) == 1 and packed["_retired"][0] is one
    assert list(packed[name]) == [key] and key == ops._scratch_key()
    want = launch(pack(), 33)
    assert len(got) == len(want) == 2
    for x, y in zip(got, want):
        assert tuple(x.shape)[0] == 33 and torch.equal(x, y)
    torch.cuda.synchronize()
    assert int(three[2].abs().sum()) == 0 and three[2].numel() == 6 and int(one[2].abs().sum()) == 0
    launch(packed, 16)
    assert packed[name][key] is three and len(packed["_retired"]) == 1 and list(packed[name]) == [key]
