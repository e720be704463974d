"""W8A8 without a GPU; the inputs tests/test_w8a8_gpu.py shares."""
import functools

import pytest
import torch

import fused_oracle as fo
import w8_oracle as w8
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.ops import hip, interface as ops, reference as ref
from ollamamq_amd.ops.quant import quantize_fp8


@functools.lru_cache(maxsize=None)
def quant_rows(kind, K):
    """33 rows: wide_rows, N(0, 1), or exact e4m3 ties (row max 448)."""
    if kind == "wide":
        return w8.wide_rows(33, K, seed=K)
    if kind == "normal":
        return fo.rand_bf16(33, K, seed=K + 1)
    t = w8.TABLE[:0x7F]                          # the positive finite codes
    mid = (t[:-1] + t[1:]) / 2
    mid = torch.cat([mid, -mid]).bfloat16()
    x = torch.stack([mid.roll(37 * m).repeat(K // 252 + 1)[:K]
                     for m in range(33)])
    x[:, 0] = 448.0
    return x


@functools.lru_cache(maxsize=None)
def real_cases():
    """{what: (x, codes, e, dq(W), order, bias, quantize_ref(x) @ dq(W))}"""
    x, w, _ = fo.gu_inputs(129, 80, 128, 0, 40.0)    # gates reach ~ +-100
    raw = {"plain": (fo.rand_bf16(200, 3584, seed=3784),
                     *w8.quantize_ref(w8.normal(1024, 3584, seed=3584)),
                     ("plain",), fo.rand_bf16(1024, scale=0.5, seed=1)),
           "gu": (x, *w8.quantize_ref(w), ("gu",), None),
           "all-codes": (fo.rand_bf16(129, 256, seed=9),
                         *w8.all_codes_weight(), ("plain",), None)}
    out = {}
    for what, (x, codes, e, dq, order, bias) in raw.items():
        want = fo.gemm_oracle(w8.quantize_ref(x)[2], dq, bias=bias)[0]
        out[what] = (x, codes, e, dq, order, bias,
                     fo.swiglu_oracle(want) if order[0] == "gu" else want)
    return out


REAL = ("plain", "gu", "all-codes")


@pytest.mark.parametrize("K", (64, 704, 4096))
@pytest.mark.parametrize("kind", ("wide", "normal", "ties"))
def test_quantize_fp8_is_the_reference_quantiser(kind, K):
    x = quant_rows(kind, K)
    for got, want in zip(quantize_fp8(x), w8.quantize_ref(x)):
        assert torch.equal(got, want)


@pytest.mark.parametrize("what", REAL)
def test_reference_and_blocked_fp32_within_budget(what):
    """Reference path and an fp32 sum in 64-wide k-blocks vs the oracle."""
    x, codes, e, dq, order, bias, want = real_cases()[what]
    gu = order[0] == "gu"
    y = ref.linear_w8a8(x, dq, bias)
    y = ref.swiglu(y) if gu else y
    fo.assert_bf16_close(y, want, what)
    pack = hip.pack_fp8_codes(codes, e, order)
    assert torch.equal(ops.linear(x, None, bias, packed=pack, act_fp8=True), y)
    xdq, acc = w8.quantize_ref(x)[2], torch.zeros(x.shape[0], dq.shape[0])
    for k in range(0, x.shape[1], 64):
        acc += xdq[:, k:k + 64].float() @ dq[:, k:k + 64].float().t()
    if bias is not None:
        acc += bias.float()
    emu = fo.swiglu_oracle(acc.double()) if gu else acc
    print(f"RATIO w8a8-emulation {what} "
          f"{fo.assert_bf16_close(emu.bfloat16(), want, what):.3f}")


def test_fp8_act_needs_resident_mode(capsys):
    m = LlamaModel(PRESETS["tiny-fp8"], device="cpu", dtype=torch.bfloat16,
                   fp8_act=True)
    assert not m.fp8_resident and not m.fp8_act
    assert "OLLAMAMQ_FP8_ACT ignored" in capsys.readouterr().err
