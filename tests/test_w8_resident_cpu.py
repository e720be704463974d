"""Pack-resident fp8 on the CPU: the switch is ignored, ops.linear with
weight=None is F.linear over the unpacked pack, weight_bytes counts packs."""
import pytest
import torch

import fused_oracle as fo
import w8_oracle as w8
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.ops import hip, interface as ops, reference as ref


def test_flag_ignored_on_cpu(monkeypatch):
    monkeypatch.setenv("OLLAMAMQ_FP8_RESIDENT", "1")
    m = LlamaModel(PRESETS["tiny-fp8"], device="cpu", dtype=torch.bfloat16)
    assert not m.fp8_resident and m.lm_head is not None
    assert all(l.wqkv is not None and l.wqkv_pk is None for l in m.layers)


@pytest.mark.parametrize("order,N", [(("plain",), 96), (("qkv", 2, 1), 512),
                                     (("gu",), 96)], ids=str)
def test_linear_without_weight(order, N):
    K = 128
    codes, e, dq = w8.quantize_ref(w8.normal(N, K, seed=N))
    pack = hip.pack_fp8_codes(codes, e, order)
    x = fo.rand_bf16(5, K, seed=1)
    bias = None if order[0] == "gu" else fo.rand_bf16(N, seed=2)
    want = torch.nn.functional.linear(x, dq, bias)
    if order[0] == "gu":
        want = ref.swiglu(want)
        assert torch.equal(ops.gateup_swiglu(x, None, pack), want)
    assert torch.equal(ops.linear(x, None, bias, packed=pack), want)
    with pytest.raises(ValueError):
        ops.linear(x, None, bias, packed=pack.codes)


def test_weight_bytes_counts_packs():
    m = LlamaModel(PRESETS["tiny-fp8"], device="cpu", dtype=torch.bfloat16)
    full = m.weight_bytes()
    (V, H), l = m.lm_head.shape, m.layers[0]
    n, k = l.wdown.shape
    m.lm_head_pk, m.lm_head = hip.pack_weight_fp8(m.lm_head), None
    l.wdown_pk, l.wdown = hip.pack_weight_fp8(l.wdown), None
    assert m.lm_head_pk.nbytes() == V * H + 4 * V
    assert m.weight_bytes() == full - (V * H - 4 * V) - (n * k - 4 * n)
