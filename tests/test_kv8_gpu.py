"""FP8 (e4m3) KV cache on the GPU (1 GPU).

Writers: the pool bytes must equal the CPU store rule (quant.kv_fp8_encode)
applied to the bf16 rows the bf16 path stores, and nothing else may move.
Readers: an e4m3 value is exact in bf16 and the kernels widen while staging,
so the output on an fp8 cache must be torch.equal to the output of the bf16
instantiation on a twin cache holding the decoded values; the same outputs
are held to the fp64 oracle with the unchanged budgets."""
import pytest
import torch

import attn_oracle as ao
import elem_oracle as eo
import fused_oracle as fo
import model_oracle as mo
import w8_oracle as w8
from ollamamq_amd.engine import GenParams, LlamaEngine, PagedKVCache
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.ops import quant, reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


def _fp8_like(c, device=DEV):
    """An fp8 cache of c's geometry and page table."""
    f = PagedKVCache(c.k_pool.shape[0], c.n_kv_heads, 128,
                     page_size=c.page_size, n_pages=c.n_pages,
                     max_slots=c.max_slots, max_ctx=c.max_ctx, device=device,
                     kv_quant="fp8")
    f.page_table.copy_(c.page_table)
    return f


def _bytes(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)


# ---------------------------------------------------------------------------
# writers


def _append_case(KVH, T, seed):
    """Adversarial append pool as an fp8 cache with seeded byte pre-fill,
    and T distinct shuffled (slot, position) pairs."""
    pool = eo.append_pool(KVH, seed)
    pairs = [(s, p) for s in range(eo.APPEND_SEQS)
             for p in range(eo.APPEND_CAP)]
    g = torch.Generator().manual_seed(seed)
    pairs = [pairs[i] for i in torch.randperm(len(pairs), generator=g)[:T]]
    slots = torch.tensor([pool.slots[s] for s, _ in pairs], dtype=torch.int32)
    pos = torch.tensor([p for _, p in pairs], dtype=torch.int32)
    f = _fp8_like(pool.cache)
    k0, v0 = _bytes(f.k_pool.shape, seed + 1), _bytes(f.k_pool.shape, seed + 2)
    f.k_pool.copy_(k0)
    f.v_pool.copy_(v0)
    return f, k0, v0, slots, pos


def _check_pool(got, before, ptab, slots, pos, rows, what):
    want = eo.pool_after(before, ptab, slots, pos, quant.kv_fp8_encode(rows))
    assert torch.equal(got.cpu(), want), what


@pytest.mark.parametrize("op", ["kv_append", "rope_append"])
def test_writers_every_bf16_pattern(op):
    hip = _hip()
    KVH, T = 4, 128
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    k = bits.view(torch.bfloat16).reshape(T, KVH, 128)
    v = k.flip(0).contiguous()
    f, k0, v0, slots, pos = _append_case(KVH, T, seed=3)
    kd, vd = k.to(DEV), v.to(DEV)
    if op == "kv_append":
        hip.kv_append(f, ao.LAYER, kd, vd, slots.to(DEV), pos.to(DEV))
    else:       # identity rotation: cos = 1, sin = 0.  The two head rows
        # with inf / NaN are zeroed in k (x * 0 is NaN there; the inf and
        # NaN rules of this writer's K branch are in test_rope_append_twin)
        cos = torch.ones(eo.APPEND_CAP, 64, device=DEV)
        q = torch.zeros(T, KVH, 128, dtype=torch.bfloat16, device=DEV)
        fin = torch.isfinite(k.float()).all(-1, keepdim=True)  # head rows
        k = torch.where(fin, k, torch.zeros_like(k))
        kd = k.to(DEV)
        hip.rope_append(f, ao.LAYER, q, kd, vd, pos.to(DEV), slots.to(DEV),
                        cos, torch.zeros_like(cos))
        # the stored row is the rotated k the kernel hands back (a -0.0
        # paired with a negative partner comes back as +0.0)
        assert torch.equal(kd.cpu(), k) and not q.any()
        k = kd.cpu()
    ptab = f.page_table.cpu()
    _check_pool(f.k_pool, k0, ptab, slots, pos, k, op + " K")
    _check_pool(f.v_pool, v0, ptab, slots, pos, v, op + " V")


def test_rope_append_twin():
    hip = _hip()
    KVH, Hq, T = 2, 6, 21
    f, k0, v0, slots, pos = _append_case(KVH, T, seed=5)
    twin = eo.append_pool(KVH, 5).to(DEV).cache
    cos, sin = (t.to(DEV) for t in fo.rope_tables(eo.APPEND_CAP))
    qkv = fo.rand_bf16(T, (Hq + 2 * KVH) * 128, scale=40.0, seed=9)
    qkv[0, Hq * 128] = float("inf")             # k rows with inf, -inf, NaN
    qkv[1, Hq * 128 + 3] = float("-inf")
    qkv[2, Hq * 128 + 130] = float("nan")
    outs = []
    for cache in (twin, f):
        buf = qkv.clone().to(DEV)
        q, k, v = (t.view(T, -1, 128) for t in buf.split(
            [Hq * 128, KVH * 128, KVH * 128], dim=1))
        hip.rope_append(cache, ao.LAYER, q, k, v, pos.to(DEV), slots.to(DEV),
                        cos, sin)
        outs.append(buf.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    ptab = f.page_table.cpu()
    for got, before, tw in ((f.k_pool, k0, twin.k_pool),
                            (f.v_pool, v0, twin.v_pool)):
        layer, pg, off = fo.paged_coords(ptab, slots, pos, ao.PAGE, ao.LAYER)
        _check_pool(got, before, ptab, slots, pos,
                    tw.cpu()[layer, pg, :, off], "rope_append twin")


@pytest.mark.parametrize("fp8w", [False, True], ids=["bf16w", "fp8w"])
@pytest.mark.parametrize("K", [64, 704])
def test_linear_qkv_rope_twin(K, fp8w):
    hip = _hip()
    nl, nkl = 4, 2
    N = (nl + 2 * nkl) * 128
    w = w8.normal(N, K, s=4.0 * K ** -0.5, seed=K)
    pack = (hip.pack_weight_qkv_rope_fp8 if fp8w
            else hip.pack_weight_qkv_rope)(w.to(DEV), nl, nkl)
    order = torch.tensor(hip.qkv_rope_order(nl, nkl))
    bias_rp = fo.rand_bf16(N, scale=0.5, seed=N)[order].contiguous().to(DEV)
    cos, sin = (t.to(DEV) for t in fo.rope_tables(fo.QKV_CTX))
    x = fo.rand_bf16(64, K, seed=K + 1)
    g = torch.Generator().manual_seed(K)
    for M in (1, 5, 32, 33, 64):
        rows = 32 * ((M + 31) // 32)
        pairs = torch.randperm(24 * fo.QKV_CTX, generator=g)[:M]
        slots, pos = (pairs // fo.QKV_CTX).int(), (pairs % fo.QKV_CTX).int()
        twin = PagedKVCache(3, nkl, 128, n_pages=24 * 8, max_slots=24,
                            max_ctx=fo.QKV_CTX, device=DEV,
                            dtype=torch.bfloat16)
        twin.page_table.copy_(torch.randperm(24 * 8, generator=g).int()
                              .reshape(24, 8))
        f = _fp8_like(twin)
        k0, v0 = _bytes(f.k_pool.shape, M), _bytes(f.k_pool.shape, M + 1)
        parts = fo.synthetic_partials(x[:M], 7, seed=M, rows=rows).to(DEV)
        for bias in (None, bias_rp):
            for frag in ((1,) if M > 32 else (0, 1)):
                xin = (fo.to_frag(x[:M], rows=rows, fill=float("nan"))
                       if frag else x[:M].contiguous()).to(DEV)
                f.k_pool.copy_(k0)
                f.v_pool.copy_(v0)
                ys = [hip.linear_qkv_rope(
                    xin, pack, N, bias, c, 1, pos.to(DEV), slots.to(DEV),
                    cos, sin, nl, nkl, parts, 7, 1.0 / K, fo.EPS,
                    **(dict(K=K, M_real=M) if frag else {}))[:, :nl * 128]
                    for c in (twin, f)]
                assert torch.equal(ys[0], ys[1]), (M, frag)
                ptab = f.page_table.cpu()
                layer, pg, off = fo.paged_coords(ptab, slots, pos, 16, 1)
                for got, before, tw in ((f.k_pool, k0, twin.k_pool),
                                        (f.v_pool, v0, twin.v_pool)):
                    want = before.clone()
                    want[layer, pg, :, off] = quant.kv_fp8_encode(
                        tw.cpu()[layer, pg, :, off])
                    assert torch.equal(got.cpu(), want), (M, frag)


# ---------------------------------------------------------------------------
# readers


def _twins(kvs, seed, max_ctx=None):
    """(cpu Pool of the snapped values, its device copy, the fp8 twin)."""
    snap = [tuple(quant.kv_fp8_decode(quant.kv_fp8_encode(t),
                                      torch.bfloat16) for t in kv)
            for kv in kvs]
    cpu = ao.build_pool(snap, seed=seed, max_ctx=max_ctx)
    f = _fp8_like(cpu.cache)
    f.k_pool.copy_(quant.kv_fp8_encode(cpu.cache.k_pool))
    f.v_pool.copy_(quant.kv_fp8_encode(cpu.cache.v_pool))
    assert int(f.k_pool[0, 0, 0, 0, 0]) == 0x7F       # unowned: NaN code
    return cpu, cpu.to(DEV), ao.Pool(f, cpu.slots, cpu.K, cpu.V)


def _same(fn, q, bf, f8, what, **meta):
    """fn on the bf16 twin and on the fp8 cache: finite and bit-equal."""
    n = len(meta["seq_lens"])
    a, b = (fn(q, p.cache, ao.LAYER, p.meta(list(range(n)), **meta)).cpu()
            for p in (bf, f8))
    assert torch.isfinite(b).all(), what
    assert torch.equal(a, b), what
    return b


def _truth(q, cpu, lens, q_lens, W):
    return ao.oracle_from_cache(q, cpu.cache, ao.LAYER, cpu.slots[:len(lens)],
                                lens, q_lens, window=W)


DEC_LENS = (1, 15, 16, 17, 63, 64, 65, 129, 200)


@pytest.mark.parametrize("G", [1, 2, 3, 4, 7, 8])
def test_decode_twin_and_oracle(G, monkeypatch):
    hip = _hip()
    runs = [(DEC_LENS, 0, (None, 1, 2, 3, 5), 512),
            (ao.CAPTURE_LENS, 0, (None,), ao.CAPTURE_MAX_KV),
            (ao.DECODE_WINDOWS[1][1], 64, (1, 3), 512)]
    for ri, (lens, W, splits, max_kv) in enumerate(runs):
        kvs, q = ao.decode_inputs(G, 2, 40 + ri, lens, 1.0)
        cpu, bf, f8 = _twins(kvs, seed=G + ri, max_ctx=max_kv)
        truth, _ = _truth(q, cpu, lens, [1] * len(lens), W)
        meta = dict(seq_lens=lens, window=W, max_kv=max_kv)
        for chunk, split, blk in [(c, s, b) for c in (32, 64)
                                  for s in splits for b in "01"]:
            monkeypatch.setattr(hip, "_CHUNK_ENV", str(chunk))
            monkeypatch.setenv("OLLAMAMQ_DECODE_BLOCKSPLIT", blk)
            monkeypatch.delenv("OLLAMAMQ_DECODE_SPLIT", raising=False)
            if split is not None:
                monkeypatch.setenv("OLLAMAMQ_DECODE_SPLIT", str(split))
            what = f"G{G} run {ri} CH{chunk} split {split} blk {blk}"
            out = _same(hip.attention_decode, q.to(DEV), bf, f8, what, **meta)
            fr = hip.attention_decode(
                q.to(DEV), f8.cache, ao.LAYER,
                f8.meta(list(range(len(lens))), **meta), fragout=True)
            assert torch.equal(fo.from_frag(fr, len(lens), 2 * G * 128).cpu()
                               .view(out.shape), out), what + " fragout"
            if blk == "0":
                ao.assert_close(out, truth, [1] * len(lens), what=what)


PRE_CASES = ((1, 1), (31, 31), (33, 33), (65, 65), (130, 130), (23, 63),
             (1, 200))
MIXED = tuple((1, n) for n in ao.MIXED_DECODE_LENS) + ao.MIXED_PREFILL


@pytest.mark.parametrize("G,W,cases", [(G, W, PRE_CASES) for G in (1, 4, 7)
                                       for W in (0, 70)] + [(4, 0, MIXED)])
def test_prefill_mixed_twin_and_oracle(G, W, cases):
    hip = _hip()
    kvs, q = ao.prefill_inputs(G, 2, 50 + W, cases, 1.0)
    cpu, bf, f8 = _twins(kvs, seed=G + W)
    q_lens, lens = [a for a, _ in cases], [b for _, b in cases]
    mixed = dict(mode="mixed", n_decode=3) if cases is MIXED else {}
    out = _same(hip.attention_mixed if mixed else hip.attention_prefill,
                q.to(DEV), bf, f8, f"G{G} W{W}", seq_lens=lens,
                q_lens=q_lens, window=W, **mixed)
    truth, absP = _truth(q, cpu, lens, q_lens, W)
    if not mixed:
        ao.assert_close(out, truth, q_lens, absP, what=f"G{G} W{W}")


# ---------------------------------------------------------------------------
# wrapper contract, model and engine


def test_wrapper_contract(monkeypatch):
    hip = _hip()
    kvs, q = ao.decode_inputs(4, 2, 70, (17, 40), 1.0)
    _, _, f8 = _twins(kvs, seed=70)
    c, qd = f8.cache, q.to(DEV)
    meta = f8.meta([0, 1], (17, 40))
    pre = f8.meta([0, 1], (17, 40), q_lens=[1, 1], mode="prefill")
    mix = f8.meta([0, 1], (17, 40), q_lens=[1, 1], mode="mixed", n_decode=1)
    k = torch.zeros(2, 2, 128, device=DEV)
    at = meta.slot_ids, meta.seq_lens - 1
    cos = torch.ones(64, 64, device=DEV)
    x = torch.zeros(2, 64, device=DEV)

    def calls(qd, k):
        return [lambda: hip.attention_decode(qd, c, ao.LAYER, meta),
                lambda: hip.attention_prefill(qd, c, ao.LAYER, pre),
                lambda: hip.attention_mixed(qd, c, ao.LAYER, mix),
                lambda: hip.kv_append(c, ao.LAYER, k, k, *at),
                lambda: hip.rope_append(c, ao.LAYER, qd, k, k, at[1], at[0],
                                        cos, cos)]
    bad = calls(qd.float(), k) + [        # fp32 rows where bf16 is required
        lambda: hip.linear_qkv_rope(x, x.bfloat16().view(-1), 1024, None, c,
                                    ao.LAYER, at[1], at[0], cos, cos, 4, 2,
                                    None, 0, 0.0, 0.0),
        lambda: hip.decode_pure(c, ao.LAYER, meta, 2)]
    for var, call in (("OLLAMAMQ_FUSED_COMBINE", calls(qd, k)[0]),
                      ("OLLAMAMQ_VALU_PREFILL", calls(qd, k)[1])):
        def switched(var=var, call=call):
            monkeypatch.setenv(var, "1")
            try:
                call()
            finally:
                monkeypatch.delenv(var)
        bad.append(switched)
    for call in bad:
        with pytest.raises(ValueError):
            call()
    pools = c.k_pool, c.v_pool
    for pool in (c.k_pool.bfloat16(), c.k_pool.transpose(3, 4)):
        c.k_pool = c.v_pool = pool
        for call in calls(qd, k.bfloat16()):
            with pytest.raises(ValueError):
                call()
    c.k_pool, c.v_pool = pools


def _cpu_logits(model, seqs):
    """Teacher-forced ops/reference.py run of a CPU model on an fp8 cache:
    logits of every position, per sequence."""
    kv = PagedKVCache.for_model(model.cfg, n_pages=sum(len(s) // 16 + 1
                                                       for s in seqs),
                                max_slots=len(seqs), max_ctx=128,
                                kv_quant="fp8")
    out = []
    for toks in seqs:
        n, slot = len(toks), kv.alloc_slot()
        kv.ensure(slot, n)
        out.append(model.forward(
            torch.tensor(toks, dtype=torch.int32),
            torch.arange(n, dtype=torch.int32), kv,
            torch.full((n,), slot, dtype=torch.int32),
            mo._prefill_meta(slot, n, 0)))
    return out


@pytest.mark.parametrize("B", mo.EXACT_B)
@pytest.mark.parametrize("name", ["tiny", "tiny-qwen"])
def test_model_forward_fp8_cache(name, B):
    """Teacher-forced prefill (one sequence of 120 tokens, the rest ragged)
    and one decode step of B rows, generic and fused, on a scrambled fp8
    cache next to a bf16 rig of the same allocation.

    Budgets (2 x the CPU bf16 run's worst rel / mx against the fp32-weights
    run, both through ops/reference.py on an fp8 cache) and the worst GPU
    ratio are printed; docs/KERNELS.md "FP8 KV cache" records them."""
    from test_model_forward_gpu import gpu_model
    ctx = (120,) + mo.decode_ctx(B)[:B - 1]
    seqs = mo.case_tokens(name, f"kv8-{B}", [c + 1 for c in ctx])
    truth = _cpu_logits(mo.upcast_model(name), seqs)
    rel, mx = (2 * float(torch.cat(m).max()) for m in zip(*(
        mo.row_metrics(r, t) for r, t in zip(
            _cpu_logits(mo.cpu_model(name), seqs), truth))))
    print(f"BUDGET kv8 {name} B={B}: rel {rel:.4f} mx {mx:.4f}"
          + (" (rel above 0.1: uninformative, mx only)" if rel > 0.1 else ""))
    rig = mo.Rig(gpu_model(name), seqs, DEV, seed=B)
    r8 = mo.Rig(gpu_model(name), seqs, DEV, seed=B)
    r8.kv = PagedKVCache.for_model(
        rig.model.cfg, n_pages=rig.kv.n_pages, max_slots=80,
        max_ctx=mo.MAX_CTX, device=DEV, kv_quant="fp8")
    mo.scramble(r8.kv, B)
    before = _bytes(r8.kv.k_pool.shape, B), _bytes(r8.kv.k_pool.shape, B + 1)
    r8.slots = [r8.kv.alloc_slot() for _ in seqs]
    assert r8.slots == rig.slots
    pre = [(i, 0, c) for i, c in enumerate(ctx)]
    dec = [(i, c, c + 1) for i, c in enumerate(ctx)]
    worst = 0.0
    for fused in (False, True):
        for r in (rig, r8):
            for pool, fill in zip((r.kv.k_pool, r.kv.v_pool), before):
                pool.copy_(fill if r is r8 else fill.bfloat16())
            r.done = [0] * len(seqs)
            got = [r.forward(pre, "prefill"),
                   r.forward(dec, "decode", fused=fused)]
        assert r8.kv._slot_pages == rig.kv._slot_pages
        own = mo.owned_mask(r8.kv, {s: c + 1 for s, c in zip(r8.slots, ctx)})
        own = own[:, None, :, None]                  # [P, 1, page, 1]
        for p8, p16, was in zip((r8.kv.k_pool, r8.kv.v_pool),
                                (rig.kv.k_pool, rig.kv.v_pool), before):
            p8 = p8.cpu()
            want0 = quant.kv_fp8_encode(p16[0].cpu())
            assert torch.equal(p8[0][own.expand_as(p8[0])],
                               want0[own.expand_as(want0)]), "layer-0 rows"
            assert not bool(((p8 != was) & ~own[None]).any()), \
                "bytes outside the owned rows changed"
        for logits, rows in got:
            want = torch.stack([truth[s][p] for s, p in rows])
            g_rel, g_mx = mo.row_metrics(logits, want)
            r_rel, r_mx = float(g_rel.max()) / rel, float(g_mx.max()) / mx
            if rel > 0.1:      # cannot fail: reported above, not asserted
                r_rel = 0.0
            assert max(r_rel, r_mx) <= 1.0, (fused, r_rel, r_mx, rel, mx)
            worst = max(worst, r_rel, r_mx)
    print(f"RATIO kv8 {name} B={B}: worst {worst:.3f}")


def test_engine_fp8_cache_paths():
    """Five sequences in bucket 6 (one pad row), lengths crossing 15 -> 16
    and 63 -> 64, on an fp8 cache: eager, graphed and pipelined decode give
    identical tokens, all through the e4m3 kernels."""
    cfg = PRESETS["tiny"]
    model = LlamaModel(cfg, device=DEV, dtype=torch.bfloat16, seed=7)
    prompts = [list(range(1, 1 + n)) for n in (12, 14, 30, 60, 62)]

    def run(graphs, pipeline):
        kv = PagedKVCache.for_model(cfg, n_pages=64, max_slots=8,
                                    max_ctx=128, device=DEV, kv_quant="fp8")
        eng = LlamaEngine(model, kv, max_batch=6)
        eng.use_graphs, eng.use_pipeline = graphs, pipeline
        seqs = [eng.seqs[eng.submit(p, GenParams(max_tokens=8))]
                for p in prompts]
        for _ in range(200):
            eng.step()
            if not eng.has_work():
                break
        assert not eng.has_work() and kv.k_pool.dtype == torch.uint8
        return [s.generated for s in seqs]

    eager = run(False, False)
    assert [len(t) for t in eager] == [8] * 5
    assert run(True, False) == eager and run(True, True) == eager
