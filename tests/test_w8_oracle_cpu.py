"""FP8 (e4m3) weight-only quantisation on the CPU: the yardstick
(tests/w8_oracle.py) is proven, then the project's quantiser, the fp8
packs, the model build and the reporting are held to it.

Requantisation.  e = ceil(log2(absmax / 448)) puts absmax / 2^e in
(224, 448].  A row whose largest |u| lies in (224, 232] rounds (ties to
even) to a largest code of exactly 224 = 448 / 2, so requantising dq finds
e - 1 and the codes of 2q: the same VALUES with the exponent moved by one.
The tests therefore assert that dq is reproduced bit for bit in every row,
that codes and exponents are reproduced in every row whose largest code is
above 224, and that the remaining rows come back as exactly (2q, e - 1) and
are a fixed point from then on.
"""
import dataclasses

import pytest
import torch

import model_oracle as mo
import w8_oracle as w8
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.models.llama import model_size_bytes, quantization_level
from ollamamq_amd.ops import hip, quant


def _inputs():
    return {
        "normal-1024x512": w8.normal(1024, 512, seed=1),
        "normal-96x704-s4": w8.normal(96, 704, s=4.0, seed=2),
        "normal-64x192-tiny": w8.normal(64, 192, s=2.0 ** -12, seed=3),
        "wide-rows": w8.wide_rows(96, 256, seed=4),
    }


INPUTS = _inputs()


# ---------------------------------------------------------------------------
# the yardstick


def test_decode_table_agrees_with_torch_on_every_finite_code():
    assert len(w8.FINITE) == 254
    c = torch.tensor(w8.FINITE, dtype=torch.uint8)
    t = c.view(torch.float8_e4m3fn).double()
    assert torch.equal(w8.decode(c), t)
    assert torch.equal(torch.signbit(w8.decode(c)), torch.signbit(t))
    assert torch.isnan(w8.TABLE[list(w8.NAN_CODES)]).all()
    assert float(w8.TABLE[0x7E]) == 448.0 and float(w8.TABLE[1]) == 2.0 ** -9
    # the project's decoder reads the same table
    assert torch.equal(quant.e4m3_decode(c).double(), w8.decode(c))


def test_row_exponent_at_the_edges():
    for p in range(-30, 31):
        assert w8.row_exponent(448.0 * 2.0 ** p) == p       # exact power
        assert w8.row_exponent(448.0 * 2.0 ** p * (1 + 2.0 ** -7)) == p + 1
        assert w8.row_exponent(448.0 * 2.0 ** p * (1 - 2.0 ** -8)) == p
    assert w8.row_exponent(0.0) == 0


# ---------------------------------------------------------------------------
# quantiser properties


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_quantiser_matches_reference(name):
    w = INPUTS[name]
    codes, e, dq = quant.quantize_fp8(w)
    rc, re_, rdq = w8.quantize_ref(w)
    assert torch.equal(e, re_)
    assert torch.equal(codes, rc)
    assert torch.equal(dq.view(torch.int16), rdq.view(torch.int16))


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_quantiser_properties(name):
    w = INPUTS[name]
    codes, e, dq = quant.quantize_fp8(w)
    scale = w8.scales(e).double()
    q = w8.decode(codes)
    # no NaN code
    assert not bool(((codes & 0x7F) == 0x7F).any())
    # dq == q * 2^e bit for bit after the bf16 cast
    assert dq.dtype == torch.bfloat16
    assert torch.equal(dq.double(), q * scale.unsqueeze(1))
    # error bound; |u| above 448 would be a clamp fault
    wd = w.double()
    u = wd / scale.unsqueeze(1)
    assert float(u.abs().max()) <= 448.0
    err = (dq.double() - wd).abs()
    big = u.abs() >= 2.0 ** -6
    assert bool((err[big] <= 2.0 ** -4 * wd.abs()[big]).all())
    lim = (2.0 ** -10 * scale).unsqueeze(1).expand_as(err)
    assert bool((err[~big] <= lim[~big]).all())
    # requantisation (module docstring)
    c2, e2, dq2 = quant.quantize_fp8(dq)
    assert torch.equal(dq2.view(torch.int16), dq.view(torch.int16))
    top = q.abs().amax(1)
    halved = (top == 224.0)
    assert bool((top[~halved & (top > 0)] > 224.0).all())
    assert torch.equal(c2[~halved], codes[~halved])
    assert torch.equal(e2[~halved], e[~halved])
    assert torch.equal(e2[halved], e[halved] - 1)
    assert torch.equal(w8.decode(c2[halved]), 2.0 * q[halved])
    c3, e3, _ = quant.quantize_fp8(dq2)
    assert torch.equal(c3, c2) and torch.equal(e3, e2)


def test_zero_row_and_power_of_two_row():
    w = INPUTS["wide-rows"]
    codes, e, dq = quant.quantize_fp8(w)
    assert int(e[1]) == 0 and not bool(codes[1].any()) \
        and not bool(dq[1].any())
    # row 2: absmax = 448 * 2^-5 exactly -> e = -5, the code of -448
    assert int(e[2]) == -5
    assert int(codes[2, w.shape[1] // 2]) == 0xFE


def test_relative_error_of_the_format():
    """N(0, 1/sqrt(K)) weights: 2.65 % relative Frobenius error."""
    w = w8.normal(1024, 512, seed=1)
    dq = quant.quantize_fp8(w)[2]
    rel = float((dq.double() - w.double()).norm() / w.double().norm())
    assert 0.024 < rel < 0.029, rel


# ---------------------------------------------------------------------------
# pack round trip


@pytest.mark.parametrize("N,K", [(32, 64), (96, 704)])
def test_pack_round_trip_plain(N, K):
    w = w8.normal(N, K, seed=N + K)
    _, e, dq = w8.quantize_ref(w)
    pk = hip.pack_weight_fp8(w)
    assert pk.codes.dtype == torch.uint8 and pk.codes.numel() == N * K
    assert torch.equal(hip.unpack_weight_fp8(pk, N, K), dq)
    assert torch.equal(pk.scale, w8.scales(e))


def test_pack_round_trip_gu():
    F, K = 32, 192
    w = w8.wide_rows(2 * F, K, seed=7)
    _, e, dq = w8.quantize_ref(w)
    pk = hip.pack_weight_gu_fp8(w)
    assert torch.equal(hip.unpack_weight_fp8(pk, 2 * F, K), dq)
    # pack row t*32 + g*16 + c is natural row g*F + t*16 + c
    rows = torch.tensor([g * F + t * 16 + c for t in range(F // 16)
                         for g in range(2) for c in range(16)])
    assert torch.equal(pk.scale, w8.scales(e)[rows])
    assert pk.scale.unique().numel() > 8      # the order is observable


@pytest.mark.parametrize("nl,nkl", [(4, 2), (7, 1)])
def test_pack_round_trip_qkv(nl, nkl):
    K = 64
    N = (nl + 2 * nkl) * 128
    w = w8.wide_rows(N, K, seed=nl)
    _, e, dq = w8.quantize_ref(w)
    pk = hip.pack_weight_qkv_rope_fp8(w, nl, nkl)
    assert torch.equal(hip.unpack_weight_fp8(pk, N, K), dq)
    rows = torch.tensor(hip.qkv_rope_order(nl, nkl))
    assert torch.equal(pk.scale, w8.scales(e)[rows])
    assert pk.scale.unique().numel() > 8


def test_pack_layout_is_the_documented_one():
    """Byte ((t*NB + b)*2 + (j >> 1))*64 + h*32 + r)*16 + (j & 1)*8 + e
    holds W[t*32 + r][b*64 + j*16 + h*8 + e] (common.cuh fp8_pack_off)."""
    N, K = 64, 192
    w = w8.normal(N, K, seed=5)
    codes = w8.quantize_ref(w)[0]
    pk = hip.pack_weight_fp8(w)
    NB = K // 64
    n = torch.arange(N).unsqueeze(1)
    k = torch.arange(K).unsqueeze(0)
    t, r = n // 32, n % 32
    b, j, h, el = k >> 6, (k >> 4) & 3, (k >> 3) & 1, k & 7
    off = ((((t * NB + b) * 2 + (j >> 1)) * 64 + h * 32 + r) * 16
           + (j & 1) * 8 + el)
    assert torch.equal(pk.codes[off.reshape(-1)].reshape(N, K), codes)


# ---------------------------------------------------------------------------
# model build


QUANTISED = ("wqkv", "wo", "wgate_up", "wdown")


def _fp8_model(**kw):
    return LlamaModel(PRESETS["tiny-fp8"], device="cpu",
                      dtype=torch.bfloat16, seed=mo.SEED, **kw)


def test_model_build_fixed_points_and_embed():
    m = _fp8_model()
    base = mo.cpu_model("tiny")
    assert torch.equal(m.embed, base.embed)
    assert m.lm_head_pk is None and all(l.wqkv_pk is None for l in m.layers)
    mats = [m.lm_head] + [getattr(l, k) for l in m.layers for k in QUANTISED]
    for w in mats:
        assert w.dtype == torch.bfloat16
        assert torch.equal(w8.quantize_ref(w)[2].view(torch.int16),
                           w.view(torch.int16))
    # and it IS quantised: every matrix differs from the bf16 preset's
    assert not torch.equal(m.lm_head, base.lm_head)
    for a, b in zip(m.layers, base.layers):
        for k in QUANTISED:
            assert not torch.equal(getattr(a, k), getattr(b, k))
            assert torch.equal(getattr(a, k),
                               w8.quantize_ref(getattr(b, k))[2])
        assert torch.equal(a.attn_norm, b.attn_norm)


def test_model_build_tp_shards_are_slices():
    cfg = PRESETS["tiny-fp8"]
    one = _fp8_model()
    Hq, KVH, d, F, V = cfg.n_heads, cfg.n_kv_heads, 128, cfg.ffn, cfg.vocab
    for rank in (0, 1):
        m = _fp8_model(tp_rank=rank, tp_size=2)
        nh, nkv, f, v = Hq // 2, KVH // 2, F // 2, V // 2
        assert torch.equal(m.lm_head, one.lm_head[rank * v:(rank + 1) * v])
        for a, g in zip(m.layers, one.layers):
            q0, k0, v0 = 0, Hq * d, (Hq + KVH) * d
            want = torch.cat([
                g.wqkv[q0 + rank * nh * d:q0 + (rank + 1) * nh * d],
                g.wqkv[k0 + rank * nkv * d:k0 + (rank + 1) * nkv * d],
                g.wqkv[v0 + rank * nkv * d:v0 + (rank + 1) * nkv * d]])
            assert torch.equal(a.wqkv, want)
            assert torch.equal(a.wo,
                               g.wo[:, rank * nh * d:(rank + 1) * nh * d])
            assert torch.equal(a.wgate_up, torch.cat([
                g.wgate_up[rank * f:(rank + 1) * f],
                g.wgate_up[F + rank * f:F + (rank + 1) * f]]))
            assert torch.equal(a.wdown, g.wdown[:, rank * f:(rank + 1) * f])


def test_unknown_quant_is_rejected():
    with pytest.raises(ValueError):
        LlamaModel(dataclasses.replace(PRESETS["tiny"], quant="int3"),
                   device="cpu", dtype=torch.bfloat16)


def test_cpu_engine_drains_a_greedy_request():
    from ollamamq_amd.engine import GenParams, LlamaEngine, PagedKVCache
    cfg = PRESETS["tiny-fp8"]
    m = _fp8_model()
    kv = PagedKVCache.for_model(cfg, n_pages=16, max_slots=2, max_ctx=64,
                                device="cpu", dtype=torch.bfloat16)
    eng = LlamaEngine(m, kv, max_batch=2)
    out = []
    eng.submit(list(range(1, 9)), GenParams(max_tokens=4, temperature=0.0),
               on_token=lambda tok, done: out.append((tok, done)))
    for _ in range(32):
        eng.step()
        if not eng.has_work():
            break
    assert not eng.has_work()
    toks = [t for t, _ in out if t >= 0]
    assert out[-1][1] and len(toks) == 4
    assert all(0 <= t < cfg.vocab for t in toks)


# ---------------------------------------------------------------------------
# presets and reporting


def test_presets_appended_after_the_existing_ones():
    names = list(PRESETS)
    first = names.index("llama3-8b-fp8")
    assert names[first:] == [
        "llama3-8b-fp8", "llama3-70b-fp8", "llama3.1-8b-fp8",
        "llama2-7b-fp8", "llama2-13b-fp8", "qwen2-7b-fp8", "mistral-7b-fp8",
        "tiny-fp8"]
    assert all(not PRESETS[n].quant for n in names[:first])
    for n in names[first:]:
        assert PRESETS[n] == dataclasses.replace(
            PRESETS[n[:-4]], name=n, quant="fp8")


def test_reported_level_and_size():
    tiny, q = PRESETS["tiny"], PRESETS["tiny-fp8"]
    assert quantization_level(tiny) == "BF16"
    assert quantization_level(q) == "FP8_E4M3"
    m = mo.cpu_model("tiny")
    assert model_size_bytes(tiny) == 2 * (m.embed.numel() + m.lm_head.numel()
                                          + sum(getattr(l, k).numel()
                                                for l in m.layers
                                                for k in QUANTISED))
    quantised = m.lm_head.numel() + sum(getattr(l, k).numel()
                                        for l in m.layers for k in QUANTISED)
    assert model_size_bytes(q) == model_size_bytes(tiny) - quantised


def test_worker_reports_quantisation():
    """/api/tags and /api/show entries of a worker offering both models;
    an exact name resolves to itself."""
    import json
    from ollamamq_amd.engine import worker as wk

    w = wk.Worker(0, models=["tiny", "tiny-fp8"])
    assert w.resolve("tiny") == "tiny" and w.resolve("tiny-fp8") == "tiny-fp8"

    class Sock:
        def __init__(self):
            self.buf = b""

        def sendall(self, b):
            self.buf += b

    conn = wk.Conn.__new__(wk.Conn)
    conn.worker, conn.sock = w, Sock()
    conn._line = lambda obj: None
    conn._meta("/api/tags", {})
    tags = {m["name"]: m for m in json.loads(conn.sock.buf)["models"]}
    assert tags["tiny"]["details"]["quantization_level"] == "BF16"
    assert tags["tiny-fp8"]["details"]["quantization_level"] == "FP8_E4M3"
    assert tags["tiny"]["size"] == model_size_bytes(PRESETS["tiny"])
    assert tags["tiny-fp8"]["size"] == model_size_bytes(PRESETS["tiny-fp8"])
    for name, level in (("tiny", "BF16"), ("tiny-fp8", "FP8_E4M3")):
        conn.sock = Sock()
        conn._meta("/api/show", {"model": name})
        assert json.loads(conn.sock.buf)["details"]["quantization_level"] \
            == level
