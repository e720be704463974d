"""W8A8 on the GPU: quantiser, GEMM and model switch against fp64 oracles."""
import functools

import pytest
import torch

import fused_oracle as fo
import model_oracle as mo
import test_w8_model_gpu as twm
import test_w8_prefill_gpu as twp
import test_w8a8_cpu as tc
import w8_oracle as w8
from ollamamq_amd.engine.kvcache import PagedKVCache
from ollamamq_amd.models import LlamaModel
from ollamamq_amd.ops import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MS = (1, 31, 32, 33, 127, 128, 129, 261)
KS = (64, 128, 384, 704)    # 128-k steps: 0.5, 1, 3 (odd), 5.5
EXACT = [(("plain",), N) for N in (32, 96, 160)] \
    + [(("qkv", nl, nkl), (nl + 2 * nkl) * 128) for nl, nkl in ((2, 1), (3, 3))] \
    + [(("gu",), 2 * F) for F in (16, 48)]


@pytest.mark.parametrize("K", (64, 704, 4096, 14336))
@pytest.mark.parametrize("kind", ("wide", "normal", "ties"))
def test_quantiser_bit_exact(kind, K):
    xa = tc.quant_rows(kind, K)
    for M in (1, 5, 33):
        x = xa[:M]
        codes, e, _ = w8.quantize_ref(x)
        buf = torch.full((M + 1, K + 24), float("nan"), dtype=torch.bfloat16)
        buf[:M, 8:8 + K] = x
        cbuf = torch.full((M + 1, K), 0xAA, dtype=torch.uint8, device=DEV)
        ebuf = torch.full((M + 1,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        c, ex = hip.quantize_act_fp8(buf.to(DEV)[:M, 8:8 + K],
                                     codes=cbuf[:M], exps=ebuf[:M])
        assert c.data_ptr() == cbuf.data_ptr()
        assert torch.equal(ex.cpu(), e), (kind, M, K)
        bad = (c.cpu() != codes).nonzero()
        assert bad.numel() == 0, (kind, M, K, bad[:4].tolist())
        assert bool((cbuf[M] == 0xAA).all()) and int(ebuf[M]) == 0x5A5A5A5A


def _pack(w, order):
    codes, e, dq = w8.quantize_ref(w)
    return hip.pack_fp8_codes(codes.to(DEV), e.to(DEV), order), dq


def _run(x, pack, N, bias=None):
    """Strided x inside a NaN buffer; NaN guard rows behind out=."""
    M, K = x.shape
    buf = torch.full((M + 1, K + 24), float("nan"), dtype=torch.bfloat16)
    buf[:M, 8:8 + K] = x
    cols = N // 2 if pack.order[0] == "gu" else N
    out = torch.full((M + 2, cols), float("nan"), dtype=torch.bfloat16,
                     device=DEV)
    guard = out[M:].clone()
    y = hip.linear_w8a8(buf.to(DEV)[:M, 8:8 + K], pack, N,
                        None if bias is None else bias.to(DEV), out=out[:M])
    assert y.data_ptr() == out.data_ptr() and y.shape == (M, cols)
    assert torch.equal(out[M:].view(torch.int16), guard.view(torch.int16))
    return y.cpu()


@pytest.mark.parametrize("order,N", EXACT, ids=str)
@pytest.mark.parametrize("K", KS)
def test_exact(K, order, N):
    """Power-of-two row scales on both sides; every sum is exact."""
    w = w8.ternary_scaled(N, K, seed=N + K)
    pack, dq = _pack(w, order)
    assert torch.equal(dq, w)
    mul = torch.ldexp(torch.ones(N), torch.arange(N, dtype=torch.int32) % 7 - 3)
    bias = (fo.int_bf16(N, lim=20, seed=N).float() * mul).bfloat16() \
        if order[0] == "qkv" else None
    xa = w8.ternary_scaled(MS[-1], K, seed=K + 1)
    if bias is not None:    # sum + bias must still fit bf16: x scales 1, 2
        xa = (fo.ternary(MS[-1], K, seed=K + 1).float()
              * (1 + torch.arange(MS[-1]) % 2).unsqueeze(1)).bfloat16()
    assert torch.equal(w8.quantize_ref(xa)[2], xa)
    for M in MS:
        x = xa[:M]
        lin = fo.gemm_oracle(x, dq, bias=bias)[0]
        assert torch.equal(lin.bfloat16().double(), lin)
        got = _run(x, pack, N, bias)
        if order[0] == "gu":        # silu is not exact; the sums are
            fo.assert_bf16_close(got, fo.swiglu_oracle(lin), f"gu M={M}")
        else:
            assert torch.equal(got.double(), lin), (M, K, order)


@pytest.mark.parametrize("what", tc.REAL)
def test_real(what):
    x, codes, e, dq, order, bias, want = tc.real_cases()[what]
    pack = hip.pack_fp8_codes(codes.to(DEV), e.to(DEV), order)
    assert torch.equal(hip.unpack_weight_fp8(pack, *codes.shape).cpu(), dq)
    got = _run(x, pack, codes.shape[0], bias)
    print(f"RATIO w8a8-real {what} "
          f"{fo.assert_bf16_close(got, want, what):.3f} "
          f"bit-equal {torch.equal(got, want.bfloat16())}")


def test_wrapper_contract():
    K, N = 128, 64
    x = fo.rand_bf16(4, K).to(DEV)
    pack, _ = _pack(w8.normal(N, K), ("plain",))
    gu, _ = _pack(w8.normal(N, K), ("gu",))
    out = torch.empty(4, N, dtype=torch.bfloat16, device=DEV)
    for args, kw in [((x.float(), pack, N), {}), ((x[:, :96], pack, N), {}),
                     ((x, pack, 48), {}),
                     ((x, gu, N, fo.rand_bf16(N).to(DEV)), {}),
                     ((x, pack, N), {"out": out[:, :32]}),
                     ((x, gu, N), {"out": out})]:
        with pytest.raises(ValueError):
            hip.linear_w8a8(*args, **kw)


@functools.lru_cache(maxsize=None)
def act_model(name):
    m = LlamaModel(twm.CONFIGS[name], device=DEV, dtype=torch.bfloat16,
                   seed=mo.SEED, fp8_resident=True, fp8_act=True)
    assert m.fp8_resident and m.fp8_act
    return m


@functools.lru_cache(maxsize=None)
def act_budget(name, tag, lens):
    """(tokens, truth, Budget of the same model through ops/reference.py:
    OLLAMAMQ_FORCE_REF, one prefill per sequence, logits everywhere)."""
    seqs, truth, _ = twm.truth_of(name, tag, lens)
    m = act_model(name)
    kv = PagedKVCache.for_model(
        m.cfg, n_pages=sum((n + mo.PAGE - 1) // mo.PAGE for n in lens),
        max_slots=len(lens), max_ctx=max(lens), device=DEV,
        dtype=torch.bfloat16)
    it = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    L, K, V = [], [], []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OLLAMAMQ_FORCE_REF", "1")
        for toks in seqs:
            n, slot = len(toks), kv.alloc_slot()
            kv.ensure(slot, n)
            L.append(m.forward(
                it(toks), it(list(range(n))), kv, it([slot] * n),
                mo._prefill_meta(slot, n, m.cfg.sliding_window, DEV)))
            K, V = K + [mo.cache_rows(kv, slot, n)[0]], \
                V + [mo.cache_rows(kv, slot, n)[1]]
    return seqs, truth, mo.Budget(mo.Obs(L, K, V), truth)


@pytest.mark.parametrize("tag,lens", mo.PREFILL_CASES[:2])
@pytest.mark.parametrize("name", sorted(twm.CONFIGS))
def test_model_prefill(name, tag, lens):
    seqs, truth, budget = act_budget(name, tag, lens)
    b = budget.fresh()
    rig = mo.Rig(act_model(name), seqs, DEV)
    logits, rows = rig.forward([(i, 0, n) for i, n in enumerate(lens)],
                               "prefill", logits_idx=len(lens) > 1)
    rig.check(truth, b, logits, rows, tag)
    lg, kv = b.report()
    print(f"RATIO w8a8-model {name} {tag} logits budget (rel, mx) "
          f"{b.lim['logits'][0]:.4f} {b.lim['logits'][1]:.4f} "
          f"used {lg:.3f} kv used {max(kv):.3f}")


@pytest.mark.parametrize("name", sorted(twm.CONFIGS))
def test_model_decode_untouched(name):
    """Fused decode B = 5 is bit-equal to the fp8_act=False model."""
    off = twp.built(name, True)[0]
    assert not off.fp8_act
    rig, _, _, parts = twm._decode_rig(off, name, 5, 5)
    state = rig.save()
    want = rig.forward(parts, "decode", fused=True)[0]
    twin = twm._decode_rig(act_model(name), name, 5, 5)[0]
    twin.restore(state)
    assert torch.equal(twin.forward(parts, "decode", fused=True)[0], want)
