"""Fused decode-chain kernels vs fp64 oracles (1 GPU).

Tier A feeds integer inputs whose every partial sum is exact in fp32 and
whose results are integers <= 256, exact in bf16: the kernel must match
the oracle with torch.equal, so a dropped or duplicated k-block, a wrong
row, tile, frag offset or combine shows as a mismatch.  Tier B feeds real
values and holds each output element to one bf16 ulp plus 2^-8 of the
tensor's rms (fused_oracle.assert_bf16_close; soundness proven on the CPU
in test_fused_oracle_cpu.py).  The worst normalised error of each tier-B
group is printed so headroom can be recorded (docs/KERNELS.md).
"""
import pytest
import torch

import fused_oracle as fo
from ollamamq_amd.engine.kvcache import PagedKVCache
from ollamamq_amd.ops import reference as ref
from ollamamq_amd.ops.interface import AttnMeta

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


def _mt_rows(M):
    return 32 * ((M + 31) // 32)


def _bits(t):
    return t.view(torch.int16)


def _sentinel(n, seed):
    """Arbitrary bf16 bit patterns (compared as bits, so NaNs are fine)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g,
                         dtype=torch.int16).view(torch.bfloat16)


def _report(group, worst):
    print(f"[fused-oracle] {group}: worst normalised error {worst:.3f}")


# ---------------------------------------------------------------------------
# tier A: exact


def _variants(M, ks):
    """(depth, xlds, yfrag, bias) combinations linear_packed accepts."""
    out = []
    for depth, xlds in ((1, 0), (2, 0), (1, 1), (1, 2)):
        for yfrag in (0, 1):
            if yfrag and (ks > 1 or (M > 32 and xlds != 2)):
                continue        # rejected: plain combine / MT2 non-frag
            for use_bias in (0, 1):
                out.append((depth, xlds, yfrag, use_bias))
    return out


@pytest.mark.parametrize("K", fo.TIER_A_K)
def test_tier_a_plain_gemm(K):
    hip = _hip()
    n_run = 0
    for N in fo.TIER_A_N:
        x, w, bias, _ = fo.tier_a_inputs(N, K)
        pk = hip.pack_weight(w.to(DEV))
        bias_d = bias.to(DEV)
        want, want_b = {}, {}
        for M in fo.TIER_A_M:
            y = fo.gemm_oracle(x[:M], w)[0]
            yb = fo.gemm_oracle(x[:M], w, bias=bias)[0]
            assert float(yb.abs().max()) <= 256 and \
                float(y.abs().max()) <= 256
            want[M], want_b[M] = y.bfloat16().to(DEV), yb.bfloat16().to(DEV)
        for M in fo.TIER_A_M:
            x_std = x[:M].contiguous().to(DEV)
            x_fr = fo.to_frag(x[:M], rows=_mt_rows(M),
                              fill=float("nan")).to(DEV)
            for ks in fo.TIER_A_KS:
                for depth, xlds, yfrag, use_bias in _variants(M, ks):
                    kw = dict(ks=ks, depth=depth, xlds=xlds, yfrag=yfrag)
                    if xlds == 2:
                        y = hip.linear_packed(x_fr, pk,
                                              bias_d if use_bias else None,
                                              N, K=K, M_frag=M, **kw)
                    else:
                        y = hip.linear_packed(x_std, pk,
                                              bias_d if use_bias else None,
                                              N, **kw)
                    got = fo.from_frag(y, M, N) if yfrag else y[:M]
                    exp = want_b[M] if use_bias else want[M]
                    assert torch.equal(got, exp), \
                        (M, N, K, ks, depth, xlds, yfrag, use_bias,
                         int((got != exp).sum()))
                    n_run += 1
    assert n_run == 786           # every accepted combination really ran


@pytest.mark.parametrize("K", fo.TIER_A_K)
def test_tier_a_fused_residual(K):
    """res in place (standard and frag layout) + sq_out, ks = 1 and the
    ks > 1 tile combine on both m-halves; frag rows >= M stay untouched."""
    hip = _hip()
    for N in fo.TIER_A_N:
        tiles = N // 32
        x, w, _, res = fo.tier_a_inputs(N, K)
        pk = hip.pack_weight(w.to(DEV))
        for M in fo.TIER_A_M:
            y, sq, _, _ = fo.gemm_oracle(x[:M], w, res=res[:M])
            assert float(y.abs().max()) <= 256 and float(sq.max()) < 2 ** 24
            y_d, sq_d = y.bfloat16().to(DEV), sq.float().to(DEV)
            rows = _mt_rows(M)
            x_std = x[:M].contiguous().to(DEV)
            x_fr = fo.to_frag(x[:M], rows=rows, fill=float("nan")).to(DEV)
            dead = _sentinel(rows * N, seed=M + N)
            live = torch.zeros(rows * N, dtype=torch.bool)
            live[fo.frag_index(M, N).reshape(-1)] = True
            r_fr0 = torch.where(live, fo.to_frag(res[:M], rows=rows), dead)
            for ks in fo.TIER_A_KS:
                tag = (M, N, K, ks)
                # frag layout, in place
                r_fr = r_fr0.to(DEV)
                sq_out = torch.full((rows, tiles), float("nan"),
                                    device=DEV)
                out = hip.linear_packed(x_fr, pk, None, N, ks=ks, xlds=2,
                                        res=r_fr, sq_out=sq_out, y=r_fr,
                                        yfrag=1, K=K, M_frag=M)
                assert out.data_ptr() == r_fr.data_ptr()
                assert torch.equal(fo.from_frag(r_fr, M, N), y_d), tag
                assert torch.equal(sq_out[:M], sq_d), tag
                keep = ~live.to(DEV)
                assert torch.equal(_bits(r_fr)[keep],
                                   _bits(r_fr0.to(DEV))[keep]), tag
                # standard layout, in place (frag x at MT=2)
                r_std = res[:M].contiguous().to(DEV)
                sq_out = torch.full((rows, tiles), float("nan"),
                                    device=DEV)
                if M <= 32:
                    hip.linear_packed(x_std, pk, None, N, ks=ks, xlds=0,
                                      res=r_std, sq_out=sq_out, y=r_std)
                else:
                    hip.linear_packed(x_fr, pk, None, N, ks=ks, xlds=2,
                                      res=r_std, sq_out=sq_out, y=r_std,
                                      K=K, M_frag=M)
                assert torch.equal(r_std, y_d), tag
                assert torch.equal(sq_out[:M], sq_d), tag


@pytest.mark.parametrize("M", [7, 31, 33, 47])
@pytest.mark.parametrize("nt", fo.RSTD_NT)
def test_tier_a_dead_rows(M, nt):
    """NaN in every frag row >= M and in the rstd partials of rows >= M:
    live outputs stay exact (the partials sum to exactly 1, rstd = 1)."""
    hip = _hip()
    N, K = 96, 704
    x, w, bias, res = fo.tier_a_inputs(N, K)
    pk = hip.pack_weight(w.to(DEV))
    rows = _mt_rows(M)
    x_fr = fo.to_frag(x[:M], rows=rows, fill=float("nan")).to(DEV)
    parts = fo.unit_partials(M, nt, seed=M + nt, rows=rows).to(DEV)
    assert torch.isnan(parts[M:]).all() or M == rows
    # rstd + bias
    want = fo.gemm_oracle(x[:M], w, bias=bias)[0]
    assert float(want.abs().max()) <= 256
    y = hip.linear_packed(x_fr, pk, bias.to(DEV), N, xlds=2, rstd=parts,
                          rstd_nt=nt, inv_h=1.0, eps=0.0, K=K, M_frag=M)
    assert torch.isfinite(y[:M].float()).all()
    assert torch.equal(y[:M], want.bfloat16().to(DEV))
    # rstd + residual + sq_out, frag in place
    want, sq, _, _ = fo.gemm_oracle(x[:M], w, res=res[:M])
    r_fr = fo.to_frag(res[:M], rows=rows, fill=float("nan")).to(DEV)
    sq_out = torch.full((rows, N // 32), float("nan"), device=DEV)
    hip.linear_packed(x_fr, pk, None, N, xlds=2, rstd=parts, rstd_nt=nt,
                      inv_h=1.0, eps=0.0, res=r_fr, sq_out=sq_out, y=r_fr,
                      yfrag=1, K=K, M_frag=M)
    assert torch.equal(fo.from_frag(r_fr, M, N), want.bfloat16().to(DEV))
    assert torch.equal(sq_out[:M], sq.float().to(DEV))


def _qkv_cache(nkl, ptab, seed):
    """3-layer pool pre-filled with a sentinel bit pattern."""
    n_pages = ptab.numel()
    kv = PagedKVCache(3, nkl, 128, page_size=16, n_pages=n_pages,
                      max_slots=fo.QKV_SLOTS, max_ctx=fo.QKV_CTX,
                      device=DEV, dtype=torch.bfloat16)
    kv.page_table.copy_(ptab)
    n = kv.k_pool.numel()
    k0 = _sentinel(n, seed).reshape(kv.k_pool.shape)
    v0 = _sentinel(n, seed + 1).reshape(kv.v_pool.shape)
    kv.k_pool.copy_(k0)
    kv.v_pool.copy_(v0)
    return kv, k0, v0


def _check_pools(kv, k0, v0, ptab, slots, pos, layer):
    """Return the addressed K/V rows [M, nkl, 128]; assert every other
    pool element (other layers included) is bit-identical to the
    sentinel."""
    _, pages, offs = fo.paged_coords(ptab, slots, pos, 16, layer)
    k1, v1 = kv.k_pool.cpu(), kv.v_pool.cpu()
    mask = torch.zeros(k1.shape, dtype=torch.bool)
    mask[layer, pages, :, offs] = True
    assert int(mask.sum()) == slots.numel() * k1.shape[2] * 128
    for new, old, name in ((k1, k0, "K"), (v1, v0, "V")):
        same = _bits(new) == _bits(old)
        assert bool(same[~mask].all()), \
            f"{name} pool changed outside the addressed rows: " \
            f"{int((~same & ~mask).sum())} elements"
    return k1[layer, pages, :, offs], v1[layer, pages, :, offs]


@pytest.mark.parametrize("nl,nkl,M,frag", [(2, 1, 31, 0), (4, 2, 64, 1),
                                           (7, 1, 33, 1), (3, 3, 7, 1)])
def test_tier_a_qkv_rope_position_zero(nl, nkl, M, frag):
    """cos = 1, sin = 0 at position 0: the pair-ordered pack, the bias
    reorder and the pool addressing, isolated from arithmetic."""
    hip = _hip()
    K = 704
    N = (nl + 2 * nkl) * 128
    x = fo.ternary(M, K, seed=M)
    w = fo.ternary(N, K, seed=N)
    bias = fo.int_bf16(N, lim=50, seed=N + 1)
    g = torch.Generator().manual_seed(nl)
    slots = torch.randperm(fo.QKV_SLOTS * 3, generator=g)[:M].int()
    n_slots = fo.QKV_SLOTS * 3
    ptab = torch.randperm(n_slots * 8, generator=g).int().reshape(n_slots, 8)
    kv = PagedKVCache(3, nkl, 128, page_size=16, n_pages=n_slots * 8,
                      max_slots=n_slots, max_ctx=fo.QKV_CTX, device=DEV,
                      dtype=torch.bfloat16)
    kv.page_table.copy_(ptab)
    k0 = _sentinel(kv.k_pool.numel(), 1).reshape(kv.k_pool.shape)
    v0 = _sentinel(kv.k_pool.numel(), 2).reshape(kv.k_pool.shape)
    kv.k_pool.copy_(k0)
    kv.v_pool.copy_(v0)
    pos = torch.zeros(M, dtype=torch.int32)
    cos, sin = fo.rope_tables(fo.QKV_CTX)
    q, k, v = fo.qkv_oracle(x, w, nl, nkl, pos, cos, sin, bias=bias)
    assert max(float(t.abs().max()) for t in (q, k, v)) <= 256
    order = torch.tensor(hip.qkv_rope_order(nl, nkl))
    pk = hip.pack_weight_qkv_rope(w.to(DEV), nl, nkl)
    xin = fo.to_frag(x, rows=_mt_rows(M), fill=float("nan")) if frag else x
    y = hip.linear_qkv_rope(
        xin.to(DEV), pk, N, bias[order].contiguous().to(DEV), kv, 1,
        pos.to(DEV), slots.to(DEV), cos.to(DEV), sin.to(DEV), nl, nkl,
        None, 0, 0.0, 0.0, **(dict(K=K, M_real=M) if frag else {}))
    assert torch.equal(y[:, :nl * 128].cpu().view(M, nl, 128), q.bfloat16())
    kg, vg = _check_pools(kv, k0, v0, ptab, slots, pos, 1)
    assert torch.equal(kg, k.bfloat16())
    assert torch.equal(vg, v.bfloat16())


# ---------------------------------------------------------------------------
# tier B: real-valued, one bf16 ulp + 2^-8 rms


@pytest.mark.parametrize("case", fo.RSTD_CASES, ids=str)
def test_tier_b_rstd_gemm(case):
    hip = _hip()
    M, N, K, nt, mode = case
    x, w, bias, res, parts = fo.rstd_inputs(M, N, K, nt)
    inv_h, eps = 1.0 / K, fo.EPS
    pk = hip.pack_weight(w.to(DEV))
    rows = _mt_rows(M)
    frag_in = M > 32 or mode == "res"
    xin = (fo.to_frag(x, rows=rows, fill=float("nan")) if frag_in
           else x).to(DEV)
    kw = dict(K=K, M_frag=M, xlds=2) if frag_in else dict(xlds=0)
    if mode == "bias":
        truth = fo.gemm_oracle(x, w, parts, inv_h, eps, bias)[0]
        y = hip.linear_packed(xin, pk, bias.to(DEV), N, rstd=parts.to(DEV),
                              rstd_nt=nt, inv_h=inv_h, eps=eps, **kw)
        worst = fo.assert_bf16_close(y[:M], truth, str(case))
    else:
        truth, sq, _, _ = fo.gemm_oracle(x, w, parts, inv_h, eps, None, res)
        r_fr = fo.to_frag(res, rows=rows, fill=float("nan")).to(DEV)
        sq_out = torch.full((rows, N // 32), float("nan"), device=DEV)
        hip.linear_packed(xin, pk, None, N, rstd=parts.to(DEV), rstd_nt=nt,
                          inv_h=inv_h, eps=eps, res=r_fr, sq_out=sq_out,
                          y=r_fr, yfrag=1, **kw)
        worst = fo.assert_bf16_close(fo.from_frag(r_fr, M, N), truth,
                                     str(case))
        fo.assert_sq_close(sq_out[:M], sq, str(case))
    _report(f"rstd_gemm {case}", worst)


@pytest.mark.parametrize("case", fo.GU_CASES, ids=str)
def test_tier_b_linear_gu(case):
    hip = _hip()
    M, F, K, nt, frag, yfrag, gscale = case
    x, w, parts = fo.gu_inputs(M, F, K, nt, gscale)
    truth = fo.gu_oracle(x, w, parts, 1.0 / K, fo.EPS)
    pk = hip.pack_weight_gu(w.to(DEV))
    assert pk is not None
    xin = (fo.to_frag(x, rows=_mt_rows(M), fill=float("nan")) if frag
           else x).to(DEV)
    act = hip.linear_gu(
        xin, pk, 2 * F, rstd=parts.to(DEV) if nt else None, rstd_nt=nt,
        inv_h=1.0 / K, eps=fo.EPS, yfrag=yfrag,
        **(dict(K=K, M_frag=M) if frag else {}))
    got = fo.from_frag(act, M, F) if yfrag else act[:M]
    _report(f"linear_gu {case}", fo.assert_bf16_close(got, truth, str(case)))


@pytest.mark.parametrize("case", fo.QKV_CASES, ids=str)
def test_tier_b_qkv_rope(case):
    hip = _hip()
    nl, nkl, K, M, use_bias, frag, nt = case
    N = (nl + 2 * nkl) * 128
    x, w, bias, parts, slots, pos, ptab = fo.qkv_inputs(nl, nkl, K, M, nt)
    cos, sin = fo.rope_tables(fo.QKV_CTX)
    b = bias if use_bias else None
    q, k, v = fo.qkv_oracle(x, w, nl, nkl, pos, cos, sin, parts, 1.0 / K,
                            fo.EPS, b)
    kv, k0, v0 = _qkv_cache(nkl, ptab, seed=nl + K)
    order = torch.tensor(hip.qkv_rope_order(nl, nkl))
    pk = hip.pack_weight_qkv_rope(w.to(DEV), nl, nkl)
    xin = fo.to_frag(x, rows=_mt_rows(M), fill=float("nan")) if frag else x
    y = hip.linear_qkv_rope(
        xin.to(DEV), pk, N,
        bias[order].contiguous().to(DEV) if use_bias else None, kv, 1,
        pos.to(DEV), slots.to(DEV), cos.to(DEV), sin.to(DEV), nl, nkl,
        parts.to(DEV) if nt else None, nt, 1.0 / K, fo.EPS,
        **(dict(K=K, M_real=M) if frag else {}))
    worst = fo.assert_bf16_close(y[:, :nl * 128].reshape(M, nl, 128), q,
                                 f"q {case}")
    kg, vg = _check_pools(kv, k0, v0, ptab, slots, pos, 1)
    worst = max(worst, fo.assert_bf16_close(kg, k, f"k {case}"),
                fo.assert_bf16_close(vg, v, f"v {case}"))
    _report(f"qkv_rope {case}", worst)


@pytest.mark.parametrize("M", [1, 33, 64])
@pytest.mark.parametrize("H", [512, 3584])
def test_tier_b_fragify_sumsq(M, H):
    hip = _hip()
    x = fo.rand_bf16(M, H, seed=M + H)
    xf, sq = hip.fragify_sumsq(x.to(DEV))
    assert torch.equal(_bits(fo.from_frag(xf, M, H).cpu()), _bits(x))
    fo.assert_sq_close(sq, (x.double() ** 2).sum(1), f"fragify {M}x{H}")


@pytest.mark.parametrize("S,Hq,KVH,short", [
    (3, 4, 2, False), (33, 4, 2, False), (64, 4, 2, False),
    (3, 8, 1, False), (33, 8, 1, False), (64, 8, 1, False),
    (33, 4, 2, True)])
def test_tier_b_attention_fragout(S, Hq, KVH, short):
    """fragout differs from the standard output only in the store
    address: bit-equal after from_frag, with split > 1 (separate combine
    kernel) and split = 1."""
    hip = _hip()
    g = torch.Generator().manual_seed(S + Hq)
    hi = 64 if short else 230
    lens = torch.randint(1, hi + 1, (S,), generator=g).tolist()
    lens[0] = hi
    pages = sum((n + 15) // 16 for n in lens)
    caches = [PagedKVCache(2, KVH, 128, page_size=16, n_pages=pages + 4,
                           max_slots=S, max_ctx=256, device=d, dtype=dt)
              for d, dt in ((DEV, torch.bfloat16), ("cpu", torch.float32))]
    slots = []
    for n in lens:
        s_g, s_c = (c.alloc_slot() for c in caches)
        assert s_g == s_c
        for c in caches:
            c.ensure(s_g, n)
        slots.append(s_g)
    kpool = fo.rand_bf16(*caches[0].k_pool.shape, scale=0.5, seed=S)
    vpool = fo.rand_bf16(*caches[0].k_pool.shape, scale=0.5, seed=S + 1)
    caches[0].k_pool.copy_(kpool)
    caches[0].v_pool.copy_(vpool)
    caches[1].k_pool.copy_(kpool.float())
    caches[1].v_pool.copy_(vpool.float())
    q = fo.rand_bf16(S, Hq, 128, scale=0.5, seed=S + 2)

    def meta(d):
        return AttnMeta(
            mode="decode",
            slot_ids=torch.tensor(slots, dtype=torch.int32, device=d),
            seq_lens=torch.tensor(lens, dtype=torch.int32, device=d),
            cu_q=torch.arange(S + 1, dtype=torch.int32, device=d),
            logits_idx=None, max_q=1, max_kv=max(lens), window=0)

    a_std = hip.attention_decode(q.to(DEV), caches[0], 1, meta(DEV))
    a_fr = hip.attention_decode(q.to(DEV), caches[0], 1, meta(DEV),
                                fragout=True)
    assert torch.equal(_bits(fo.from_frag(a_fr, S, Hq * 128)),
                       _bits(a_std.view(S, Hq * 128)))
    want = ref.attention(q.float(), caches[1], 1, meta("cpu"))
    torch.testing.assert_close(a_std.float().cpu(), want, atol=3e-2,
                               rtol=3e-2)


@pytest.mark.parametrize("M", [5, 40])
@pytest.mark.parametrize("H", [512, 3584])
def test_tier_b_mini_layer_handoff(H, M):
    """One layer of the chain with production strides; every op is
    checked against an oracle fed with the previous op's ACTUAL device
    output, so errors do not compound and the single-rounding tolerance
    holds.  Pins the producer/consumer contract: m-major [M][tiles]
    partials, second-half offsets, in-place safety."""
    hip = _hip()
    nl, nkl, F, V = 4, 2, 1024, 512
    tiles_h = H // 32
    inv_h, eps = 1.0 / H, fo.EPS
    Nq = (nl + 2 * nkl) * 128
    s = H + M
    wqkv = fo.rand_bf16(Nq, H, scale=H ** -0.5, seed=s + 1)
    wo = fo.rand_bf16(H, nl * 128, scale=(nl * 128) ** -0.5, seed=s + 2)
    wgu = fo.rand_bf16(2 * F, H, scale=H ** -0.5, seed=s + 3)
    wdown = fo.rand_bf16(H, F, scale=F ** -0.5, seed=s + 4)
    wlm = fo.rand_bf16(V, H, scale=H ** -0.5, seed=s + 5)
    emb = fo.rand_bf16(M, H, seed=s + 6)
    attn = fo.rand_bf16(M, nl * 128, seed=s + 7)
    _, _, _, _, slots, pos, ptab = fo.qkv_inputs(nl, nkl, 256, M, 0, seed=s)
    cos, sin = fo.rope_tables(fo.QKV_CTX)
    kv, k0, v0 = _qkv_cache(nkl, ptab, seed=s)
    res = torch.zeros(64 * H, dtype=torch.bfloat16, device=DEV)
    sq_a = torch.zeros(tiles_h * 64, device=DEV)
    sq_b = torch.zeros_like(sq_a)
    worst = {}

    # 1. fragify + per-row sum of squares (one partial per row)
    hip.fragify_sumsq(emb.to(DEV), xf=res, sq=sq_a[:M])
    x0 = fo.from_frag(res, M, H).cpu()
    assert torch.equal(_bits(x0), _bits(emb))
    fo.assert_sq_close(sq_a[:M], (emb.double() ** 2).sum(1), "fragify")
    # 2. qkv + rope + append, rstd from the nt=1 partials
    p1 = sq_a[:_mt_rows(M)].cpu().reshape(-1, 1)
    q, k, v = fo.qkv_oracle(x0, wqkv, nl, nkl, pos, cos, sin, p1, inv_h,
                            eps)
    y = hip.linear_qkv_rope(
        res, hip.pack_weight_qkv_rope(wqkv.to(DEV), nl, nkl), Nq, None, kv,
        1, pos.to(DEV), slots.to(DEV), cos.to(DEV), sin.to(DEV), nl, nkl,
        sq_a, 1, inv_h, eps, K=H, M_real=M)
    worst["qkv"] = fo.assert_bf16_close(
        y[:, :nl * 128].reshape(M, nl, 128), q, "q")
    kg, vg = _check_pools(kv, k0, v0, ptab, slots, pos, 1)
    fo.assert_bf16_close(kg, k, "k")
    fo.assert_bf16_close(vg, v, "v")
    assert torch.equal(_bits(fo.from_frag(res, M, H).cpu()), _bits(x0))
    # 3. o GEMM, in place on res, emits sq_b
    truth, sq, _, _ = fo.gemm_oracle(attn, wo, res=x0)
    hip.linear_packed(fo.to_frag(attn, rows=_mt_rows(M)).to(DEV),
                      hip.pack_weight(wo.to(DEV)), None, H, ks=1, res=res,
                      sq_out=sq_b, y=res, yfrag=1, K=nl * 128, xlds=2,
                      M_frag=M)
    x1 = fo.from_frag(res, M, H).cpu()
    worst["o"] = fo.assert_bf16_close(x1, truth, "o")
    p2 = sq_b[:_mt_rows(M) * tiles_h].cpu().reshape(-1, tiles_h)
    fo.assert_sq_close(p2[:M], sq, "o sq")
    # 4. gate_up + SwiGLU, rstd from the o GEMM's partials
    truth = fo.gu_oracle(x1, wgu, p2, inv_h, eps)
    act = hip.linear_gu(res, hip.pack_weight_gu(wgu.to(DEV)), 2 * F,
                        rstd=sq_b, rstd_nt=tiles_h, inv_h=inv_h, eps=eps,
                        K=H, yfrag=1, M_frag=M)
    a1 = fo.from_frag(act, M, F).cpu()
    worst["gu"] = fo.assert_bf16_close(a1, truth, "gu")
    # 5. down GEMM, ks=2 tile combine, in place, emits sq_a
    truth, sq, _, _ = fo.gemm_oracle(a1, wdown, res=x1)
    hip.linear_packed(act, hip.pack_weight(wdown.to(DEV)), None, H, ks=2,
                      res=res, sq_out=sq_a, y=res, yfrag=1, K=F, xlds=2,
                      M_frag=M)
    x2 = fo.from_frag(res, M, H).cpu()
    worst["down"] = fo.assert_bf16_close(x2, truth, "down")
    p3 = sq_a[:_mt_rows(M) * tiles_h].cpu().reshape(-1, tiles_h)
    fo.assert_sq_close(p3[:M], sq, "down sq")
    # 6. lm_head with rstd from the down GEMM's partials
    truth = fo.gemm_oracle(x2, wlm, p3, inv_h, eps)[0]
    logits = hip.linear_packed(res, hip.pack_weight(wlm.to(DEV)), None, V,
                               rstd=sq_a, rstd_nt=tiles_h, inv_h=inv_h,
                               eps=eps, K=H, xlds=2, M_frag=M)
    worst["lm_head"] = fo.assert_bf16_close(logits[:M], truth, "lm_head")
    _report(f"mini_layer H={H} M={M}",
            max(worst.values()))
    print(f"[fused-oracle] mini_layer H={H} M={M} per op: "
          + ", ".join(f"{k}={v:.3f}" for k, v in worst.items()))


# ---------------------------------------------------------------------------
# wrapper contract: a combination either computes the oracle or raises
# before anything is launched


@pytest.mark.parametrize("combo", ["bias_ks2_res", "qkv_std_m_over_32",
                                   "sq_out_without_res", "ks2_yfrag_plain"])
def test_wrapper_contract(combo):
    hip = _hip()
    M, N, K = 7, 96, 704
    x, w, bias, res = fo.tier_a_inputs(N, K)
    x = x[:M].contiguous()
    res = res[:M].contiguous()
    pk = hip.pack_weight(w.to(DEV))
    x_fr = fo.to_frag(x, rows=32).to(DEV)
    canary = torch.full((32 * N,), 7.0, dtype=torch.bfloat16, device=DEV)
    sq_out = torch.full((32, N // 32), -1.0, device=DEV)

    def untouched():
        torch.cuda.synchronize()
        return bool((canary == 7.0).all()) and bool((sq_out == -1.0).all())

    if combo == "bias_ks2_res":
        want, sq, _, _ = fo.gemm_oracle(x, w, bias=bias, res=res)
        y = canary[:M * N].view(M, N)
        try:
            r = res.to(DEV)
            hip.linear_packed(x.to(DEV), pk, bias.to(DEV), N, ks=2, xlds=0,
                              res=r, sq_out=sq_out, y=y)
        except ValueError:
            assert untouched()
            return
        assert torch.equal(y, want.bfloat16().to(DEV))
        assert torch.equal(sq_out[:M], sq.float().to(DEV))
    elif combo == "qkv_std_m_over_32":
        nl, nkl, M2 = 2, 1, 40
        x2, w2, _, _, slots, pos, ptab = fo.qkv_inputs(nl, nkl, 256, M2, 0)
        cos, sin = fo.rope_tables(fo.QKV_CTX)
        kv, k0, v0 = _qkv_cache(nkl, ptab, seed=3)
        try:
            y = hip.linear_qkv_rope(
                x2.to(DEV), hip.pack_weight_qkv_rope(w2.to(DEV), nl, nkl),
                512, None, kv, 1, pos.to(DEV), slots.to(DEV), cos.to(DEV),
                sin.to(DEV), nl, nkl, None, 0, 0.0, 0.0)
        except ValueError:
            torch.cuda.synchronize()
            assert torch.equal(_bits(kv.k_pool.cpu()), _bits(k0))
            assert torch.equal(_bits(kv.v_pool.cpu()), _bits(v0))
            return
        q, k, v = fo.qkv_oracle(x2, w2, nl, nkl, pos, cos, sin)
        fo.assert_bf16_close(y[:, :256].reshape(M2, nl, 128), q, "q")
        kg, vg = _check_pools(kv, k0, v0, ptab, slots, pos, 1)
        fo.assert_bf16_close(kg, k, "k")
        fo.assert_bf16_close(vg, v, "v")
    elif combo == "sq_out_without_res":
        want, sq, _, _ = fo.gemm_oracle(x, w)
        y = canary[:M * N].view(M, N)
        try:
            hip.linear_packed(x.to(DEV), pk, None, N, ks=1, xlds=0,
                              sq_out=sq_out, y=y)
        except ValueError:
            assert untouched()
            return
        assert torch.equal(y, want.bfloat16().to(DEV))
        assert torch.equal(sq_out[:M], sq.float().to(DEV))
    else:
        want = fo.gemm_oracle(x, w)[0]
        try:
            hip.linear_packed(x_fr, pk, None, N, ks=2, xlds=2, yfrag=1,
                              y=canary, K=K, M_frag=M)
        except ValueError:
            assert untouched()
            return
        assert torch.equal(fo.from_frag(canary, M, N),
                           want.bfloat16().to(DEV))
