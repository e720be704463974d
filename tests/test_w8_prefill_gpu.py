"""ops.hip.linear_w8 against the fp64 oracle over dq(W) (exact, every code,
real, wrapper contract) and pack-resident fp8 models against their
non-resident twin and the fp64 model oracle (1 GPU)."""
import functools

import pytest
import torch

import fused_oracle as fo
import model_oracle as mo
import test_engine_oracle_gpu as teo
import test_w8_model_gpu as twm
import w8_oracle as w8
from ollamamq_amd.models import LlamaModel
from ollamamq_amd.ops import hip

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BM, BN = hip.W8_BM, hip.W8_BN
MS = (1, 31, 32, 33, BM - 1, BM, BM + 1, 2 * BM + 5)
# (order, N): plain N, qkv (nl, nkl) at head_dim 128, gu F = N / 2
EXACT = [(("plain",), N) for N in (32, 96, BN + 32)] \
    + [(("qkv", nl, nkl), (nl + 2 * nkl) * 128) for nl, nkl in ((2, 1), (3, 3))] \
    + [(("gu",), 2 * F) for F in (16, 48)]


def _pack(w, order):
    codes, e, dq = w8.quantize_ref(w)       # the independent quantiser
    return hip.pack_fp8_codes(codes.to(DEV), e.to(DEV), order), dq


def _run(x, pack, N, bias=None):
    """x is a strided view of a NaN buffer (row M too); out= has NaN guard
    rows that must keep their bits."""
    M, K = x.shape
    buf = torch.full((M + 1, K + 24), float("nan"), dtype=torch.bfloat16)
    buf[:M, 8:8 + K] = x
    cols = N // 2 if pack.order[0] == "gu" else N
    out = torch.full((M + 2, cols), float("nan"), dtype=torch.bfloat16, device=DEV)
    guard = out[M:].clone()
    y = hip.linear_w8(buf.to(DEV)[:M, 8:8 + K], pack, N,
                      None if bias is None else bias.to(DEV), out=out[:M])
    assert y.data_ptr() == out.data_ptr() and y.shape == (M, cols)
    assert torch.equal(out[M:].view(torch.int16), guard.view(torch.int16))
    return y.cpu()


@pytest.mark.parametrize("order,N", EXACT, ids=str)
@pytest.mark.parametrize("K", (64, 128, 704))
def test_exact(K, order, N):
    w = w8.ternary_scaled(N, K, seed=N + K)
    pack, dq = _pack(w, order)
    assert torch.equal(dq, w)
    mul = torch.ldexp(torch.ones(N), torch.arange(N, dtype=torch.int32) % 7 - 3)
    bias = (fo.int_bf16(N, lim=20, seed=N).float() * mul).bfloat16() \
        if order[0] == "qkv" else None
    xa = fo.ternary(MS[-1], K, seed=K)
    for M in MS:
        x = xa[:M]
        lin = fo.gemm_oracle(x, dq, bias=bias)[0]
        q = lin / mul.double()
        assert torch.equal(q, q.round()) and float(q.abs().max()) <= 256
        got = _run(x, pack, N, bias)
        if order[0] == "gu":        # silu is not exact; the sums are
            fo.assert_bf16_close(got, fo.swiglu_oracle(lin), f"gu M={M}")
        else:
            assert torch.equal(got.double(), lin), (M, K, order)


def test_every_code():
    codes, e, dq = w8.all_codes_weight()
    N, K = codes.shape
    pack = hip.pack_fp8_codes(codes.to(DEV), e.to(DEV))
    M = BM + 1
    for k0 in (0, M):
        cols = (k0 + torch.arange(M)) % K
        x = torch.zeros(M, K, dtype=torch.bfloat16)
        x[torch.arange(M), cols] = 1.0
        assert torch.equal(_run(x, pack, N), dq[:, cols].t().contiguous())


# (M, K, plain N, gate scale of the gu case)
REAL = [(33, 704, 96, 1.0), (BM + 1, 128, BN + 32, 40.0),
        (2 * BM + 5, 704, 32, 1.0), (200, 3584, 1024, 1.0)]


@pytest.mark.parametrize("M,K,N,gscale", REAL)
def test_real(M, K, N, gscale):
    x = fo.rand_bf16(M, K, seed=M + K)
    big = K == 3584
    for order, n in ((("plain",), N), (("gu",), 1024 if big else 96),
                     (("qkv", 3, 3), 1152) if big else (("qkv", 2, 1), 512)):
        w = w8.normal(n, K, seed=n + K)
        if order[0] == "gu" and gscale != 1.0:      # gates reach ~ +-100
            x, w, _ = fo.gu_inputs(M, n // 2, K, 0, gscale)
        pack, dq = _pack(w, order)
        bias = fo.rand_bf16(n, scale=0.5, seed=n) if order[0] != "gu" else None
        want = fo.gemm_oracle(x, dq, bias=bias)[0]
        if order[0] == "gu":
            want = fo.swiglu_oracle(want)
        fo.assert_bf16_close(_run(x, pack, n, bias), want, f"{order} M={M}")


def test_wrapper_contract():
    K, N = 128, 64
    x = fo.rand_bf16(4, K).to(DEV)
    pack, _ = _pack(w8.normal(N, K), ("plain",))
    gu, _ = _pack(w8.normal(N, K), ("gu",))
    out = torch.empty(4, N, dtype=torch.bfloat16, device=DEV)
    for args, kw in [((x, pack.codes, N), {}), ((x.float(), pack, N), {}),
                     ((x.t().contiguous().t(), pack, N), {}),
                     ((x[:, :96], pack, N), {}), ((x, pack, 48), {}),
                     ((x, gu, N, fo.rand_bf16(N).to(DEV)), {}),
                     ((x, pack, N), {"out": out[:, :32]}),
                     ((x, gu, N), {"out": out})]:
        with pytest.raises(ValueError):
            hip.linear_w8(*args, **kw)


@functools.lru_cache(maxsize=None)
def built(name, resident):
    """(model, bytes its build left allocated); scratch uploaded first."""
    cfg = twm.CONFIGS[name]
    hip.w8_colmap(cfg.n_heads, cfg.n_kv_heads, torch.device(DEV))
    before = torch.cuda.memory_allocated(DEV)
    m = LlamaModel(cfg, device=DEV, dtype=torch.bfloat16, seed=mo.SEED,
                   fp8_resident=resident)
    assert m.fused_chain and m.fp8_resident == resident
    return m, torch.cuda.memory_allocated(DEV) - before


@pytest.mark.parametrize("name", sorted(twm.CONFIGS))
def test_resident_build(name):
    (r, r_bytes), (t, t_bytes) = built(name, True), built(name, False)
    dropped = t.lm_head.numel() * 2
    assert r.lm_head is None
    pairs = [(r.lm_head_pk, t.lm_head_pk)]
    for a, b in zip(r.layers, t.layers):
        assert all(getattr(a, k) is None for k in twm.MATS)
        dropped += sum(getattr(b, k).numel() * 2 for k in twm.MATS)
        pairs += [(getattr(a, k), getattr(b, k))
                  for k in ("wqkv_pk", "wo_pk", "wgu_pk", "wdown_pk")]
    for p, q in pairs:
        assert p.order == q.order and torch.equal(p.codes, q.codes) \
            and torch.equal(p.scale, q.scale)
    assert t_bytes - r_bytes >= dropped, (t_bytes, r_bytes, dropped)
    assert t.weight_bytes() - r.weight_bytes() \
        == dropped - sum(p.nbytes() for p, _ in pairs)


@pytest.mark.parametrize("tag,lens", mo.PREFILL_CASES[:2])
@pytest.mark.parametrize("name", sorted(twm.CONFIGS))
def test_resident_prefill(name, tag, lens):
    rig, truth, b = twm._rig(built(name, True)[0], name, tag, lens)
    logits, rows = rig.forward([(i, 0, n) for i, n in enumerate(lens)],
                               "prefill", logits_idx=len(lens) > 1)
    rig.check(truth, b, logits, rows, tag)


@pytest.mark.parametrize("name", sorted(twm.CONFIGS))
def test_resident_decode(name):
    """Fused B = 5 is bit-equal to the twin from the same cache state;
    generic B = 65 runs linear_w8 everywhere."""
    res = built(name, True)[0]
    rig, truth, b, parts = twm._decode_rig(res, name, 5, 5)
    state = rig.save()
    logits, rows = rig.forward(parts, "decode", fused=True)
    rig.check(truth, b, logits, rows, "fused B=5")
    pools = mo.snapshot(rig.kv)
    twin, _, _, _ = twm._decode_rig(built(name, False)[0], name, 5, 5)
    assert twin.slots == rig.slots
    twin.restore(state)
    assert torch.equal(twin.forward(parts, "decode", fused=True)[0], logits)
    assert all(torch.equal(a, b2)
               for a, b2 in zip(mo.snapshot(twin.kv), pools))
    rig, truth, b, parts = twm._decode_rig(res, name, 65, 65)
    logits, rows = rig.forward(parts, "decode", fused=False)
    rig.check(truth, b, logits, rows, "generic B=65")


def test_resident_engine(monkeypatch):
    name = "tiny-fp8"
    monkeypatch.setattr(teo, "gpu_model", lambda n: built(n, True)[0])
    eng = teo._engine(name, seed=4)
    tap = teo.Tap(eng)
    seqs = teo._submit(eng, mo.case_tokens(name, "engine", (10, 58, 30)),
                       [teo._greedy(24)] * 3)
    teo._drive(eng)
    assert all(len(s.generated) == 24 for s in seqs)
    teo._check(name, tap, seqs, "resident w8")
