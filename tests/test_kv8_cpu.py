"""FP8 (e4m3) KV cache, CPU side: the store rule over every bf16 pattern,
the reference attention on an fp8 cache, the CPU engine and the worker's
OLLAMAMQ_KV_CACHE_TYPE switch."""
import pytest
import torch

import w8_oracle
from ollamamq_amd.engine import GenParams, LlamaEngine, PagedKVCache
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.ops import quant, reference as ref
from ollamamq_amd.ops.interface import AttnMeta


def all_bf16():
    """Every bf16 bit pattern as [512, 1, 128]: row t holds t*128 .. +127."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(512, 1, 128)


def fp8_cache(n_pages=32, **kw):
    return PagedKVCache(1, 1, 128, n_pages=n_pages, max_slots=2, max_ctx=512,
                        kv_quant="fp8", **kw)


def test_store_rule_exhaustive():
    x = all_bf16()
    cache = fp8_cache()
    assert cache.kv_fp8 and cache.k_pool.dtype == torch.uint8
    cache.ensure(0, 512)
    slot, pos = torch.zeros(512, dtype=torch.int32), torch.arange(512)
    ref.kv_append(cache, 0, x, x.flip(0), slot, pos)
    k, v = ref._gather_kv(cache, 0, 0, 512)
    pages = cache.page_table[0, :32].long()
    codes = cache.k_pool[0, pages].permute(0, 2, 1, 3).reshape(-1)
    assert torch.equal(cache.v_pool[0, pages].permute(0, 2, 1, 3)
                       .reshape(512, 128).flip(0).reshape(-1), codes)
    xf = x.reshape(-1).double()
    fin = torch.isfinite(xf)
    # brute-force nearest over the 254 finite table values, ties to the
    # even code (adjacent finite codes differ in their low bit)
    tab = w8_oracle.TABLE[w8_oracle.FINITE]
    cl = xf[fin].clamp(-448.0, 448.0)
    dist = (cl[:, None] - tab[None, :]).abs()
    best = dist.min(dim=1).values
    got = w8_oracle.decode(codes[fin])
    assert torch.equal((got - cl).abs(), best)
    tied = (dist == best[:, None]).sum(1) > 1
    nonzero = tied & (cl != 0)           # +0 / -0 share a value, not a tie
    assert nonzero.any() and bool((codes[fin][nonzero] & 1 == 0).all())
    bits = torch.arange(65536)
    assert codes[0x8000] == 0x80 and codes[0] == 0          # -0.0, +0.0
    assert bool((codes[(bits & 0x7FFF) == 0] & 0x7F == 0).all())
    assert codes[0x7F80] == 0x7E and codes[0xFF80] == 0xFE  # +-inf
    nan = torch.isnan(xf)
    assert bool((codes[nan] & 0x7F == 0x7F).all())
    assert bool((codes[fin] & 0x7F != 0x7F).all())
    # load rule and round trip
    assert torch.equal(torch.isnan(k.reshape(-1)), nan)
    assert torch.equal(k.reshape(-1)[fin].double(), got)
    every = torch.arange(256, dtype=torch.uint8)
    dec = quant.kv_fp8_decode(every, torch.bfloat16)
    assert torch.equal(dec.double()[w8_oracle.FINITE], tab)
    assert torch.equal(quant.kv_fp8_encode(dec)[w8_oracle.FINITE],
                       every[w8_oracle.FINITE])


def test_kv_quant_validated():
    with pytest.raises(ValueError):
        PagedKVCache(1, 1, 128, kv_quant="q4")
    assert not PagedKVCache(1, 1, 128, n_pages=2).kv_fp8


@pytest.mark.parametrize("qlen,kv_len", [(1, 37), (21, 37)])
def test_reference_attention_twin(qlen, kv_len):
    g = torch.Generator().manual_seed(qlen)
    twin = PagedKVCache(1, 2, 128, n_pages=8, max_slots=2, max_ctx=64)
    cache = PagedKVCache(1, 2, 128, n_pages=8, max_slots=2, max_ctx=64,
                         kv_quant="fp8")
    k = torch.randn(kv_len, 2, 128, generator=g) * 3
    v = torch.randn(kv_len, 2, 128, generator=g) * 3
    slot, pos = torch.zeros(kv_len, dtype=torch.int32), torch.arange(kv_len)
    for c in (twin, cache):
        c.alloc_slot()
        c.ensure(0, kv_len)
    ref.kv_append(cache, 0, k, v, slot, pos)
    kd, vd = ref._gather_kv(cache, 0, 0, kv_len)
    assert not torch.equal(kd, k)
    ref.kv_append(twin, 0, kd, vd, slot, pos)
    q = torch.randn(qlen, 4, 128, generator=g)
    meta = AttnMeta(mode="decode" if qlen == 1 else "prefill",
                    slot_ids=torch.tensor([0], dtype=torch.int32),
                    seq_lens=torch.tensor([kv_len], dtype=torch.int32),
                    cu_q=torch.tensor([0, qlen], dtype=torch.int32),
                    logits_idx=None, max_q=qlen, max_kv=kv_len)
    assert torch.equal(ref.attention(q, cache, 0, meta),
                       ref.attention(q, twin, 0, meta))


def test_cpu_engine_fp8_cache():
    cfg = PRESETS["tiny"]
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=7)

    def run():
        kv = PagedKVCache.for_model(cfg, n_pages=32, max_slots=4,
                                    max_ctx=128, kv_quant="fp8")
        assert kv.kv_fp8
        eng = LlamaEngine(model, kv, max_batch=4)
        seqs = [eng.seqs[eng.submit([5, 6, 7, 8], GenParams(max_tokens=6))],
                eng.seqs[eng.submit([1, 2, 3], GenParams(
                    max_tokens=6, temperature=0.9, seed=1234))]]
        for _ in range(64):
            eng.step()
            if not eng.has_work():
                break
        assert not eng.has_work()
        assert kv.k_pool.dtype == torch.uint8 and bool(kv.k_pool.any())
        return [s.generated for s in seqs]

    a = run()
    assert a == run() and [len(t) for t in a] == [6, 6]


@pytest.mark.parametrize("value,fp8", [(None, False), ("bf16", False),
                                       ("fp8", True), ("q4", None)])
def test_worker_kv_cache_type(monkeypatch, value, fp8):
    from ollamamq_amd.engine import worker as wk
    if value is None:
        monkeypatch.delenv("OLLAMAMQ_KV_CACHE_TYPE", raising=False)
    else:
        monkeypatch.setenv("OLLAMAMQ_KV_CACHE_TYPE", value)
    w = wk.Worker(0, models=["tiny"], max_batch=2, default_ctx=64)
    err = w.load("tiny", 64)
    if fp8 is None:
        assert isinstance(err, str) and "q4" in err and not w.engines
    else:
        assert err is None
        assert w.engines["tiny"].kv.kv_fp8 is fp8
