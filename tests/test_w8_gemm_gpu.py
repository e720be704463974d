"""FP8 (e4m3) weight packs through the weight-streaming kernels (1 GPU).

Four tiers, all calling ops.hip directly:
  codes   every finite e4m3 code, every row scale, through the kernel with
          one-hot activations: the output must equal the decode table.
  bits    the fp8 pack of W against the bf16 pack of dq(W) with the same
          explicit (ks, depth, xlds, yfrag, M): outputs, sq partials and
          both KV pools bit for bit.  The scale is a power of two and
          multiplies the reduced sum, which commutes with every fp32
          rounding, so equality is designed; a mismatch is a finding about
          accumulation order.
  exact   ternary x, ternary W with row n times 2^(n % 7 - 3), against the
          fp64 oracle on dq with torch.equal: a scale taken in natural
          instead of pack order moves a result by a factor >= 2.
  real    N(0, 1/sqrt(K)) weights against the fp64 oracle on dq within
          fused_oracle's unchanged budget (the kernel sees bf16-exact
          weights).
"""
import pytest
import torch

import fused_oracle as fo
import w8_oracle as w8
import test_fused_epilogues_gpu as tfe
from ollamamq_amd.engine.kvcache import PagedKVCache

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KS = (64, 256, 704, 1536, 3584)
NS = (32, 96, 1024)
MS = (1, 5, 32, 33, 64)
KSPLIT = (1, 2, 3, 8)

_hip = tfe._hip
_bits = tfe._bits
_rows = tfe._mt_rows


def _both_packs(hip, w, kind="plain", nl=0, nkl=0):
    """(fp8 pack of w, bf16 pack of dq(w), dq): the device quantiser must
    land on the reference quantiser's values."""
    _, _, dq = w8.quantize_ref(w)
    wd, dqd = w.to(DEV), dq.to(DEV)
    if kind == "gu":
        p8, p16 = hip.pack_weight_gu_fp8(wd), hip.pack_weight_gu(dqd)
    elif kind == "qkv":
        p8 = hip.pack_weight_qkv_rope_fp8(wd, nl, nkl)
        p16 = hip.pack_weight_qkv_rope(dqd, nl, nkl)
    else:
        p8, p16 = hip.pack_weight_fp8(wd), hip.pack_weight(dqd)
    assert p8 is not None and p16 is not None
    assert torch.equal(hip.unpack_weight_fp8(p8, *w.shape).cpu(), dq)
    return p8, p16, dq


# ---------------------------------------------------------------------------
# codes


@pytest.mark.parametrize("xlds", [0, 1, 2])
def test_every_code_through_the_kernel(xlds):
    hip = _hip()
    codes, e, dq = w8.all_codes_weight()
    N, K = codes.shape
    pk = hip.pack_fp8_codes(codes.to(DEV), e.to(DEV))
    M = 32 if xlds == 1 else 64
    seen = torch.zeros(K, dtype=torch.bool)
    for k0 in range(0, K, M):
        x = torch.zeros(M, K, dtype=torch.bfloat16)
        x[torch.arange(M), k0 + torch.arange(M)] = 1.0
        if xlds == 2:
            y = hip.linear_packed(fo.to_frag(x, rows=M).to(DEV), pk, None, N,
                                  ks=1, depth=1, xlds=2, K=K, M_frag=M)
        else:
            y = hip.linear_packed(x.to(DEV), pk, None, N, ks=1, depth=1,
                                  xlds=xlds)
        want = dq[:, k0:k0 + M].t().contiguous()
        assert torch.equal(y[:M].cpu(), want), (xlds, k0)
        seen[k0:k0 + M] = True
    assert bool(seen.all())
    # every finite code sat in every row, so every (code, scale) pair ran
    assert sorted(set(codes[0].tolist())) == sorted(set(w8.FINITE))


# ---------------------------------------------------------------------------
# bits


def _plain_variants(M, ks):
    """(xlds, yfrag, mode): mode in bias / none / res (res + sq_out) /
    rstd (rstd + bias, ks == 1)."""
    out = []
    for xlds in (0, 1, 2):
        if xlds == 1 and M > 32:
            continue
        for yfrag in (0, 1):
            if yfrag and (ks > 1 or (M > 32 and xlds != 2)):
                continue
            out += [(xlds, yfrag, "bias"), (xlds, yfrag, "none")]
    out.append((2, 1, "res"))
    if M <= 32:
        out.append((0, 0, "res"))
    if ks == 1:
        out += [(2, 0, "rstd"), (2, 1, "rstd")]
        if M <= 32:
            out.append((0, 0, "rstd"))
    return out


@pytest.mark.parametrize("K", KS)
def test_bits_linear_packed(K):
    hip = _hip()
    n_run = 0
    for N in NS:
        w = w8.normal(N, K, seed=N + K)
        p8, p16, _ = _both_packs(hip, w)
        x = fo.rand_bf16(64, K, seed=K + 2)
        bias = fo.rand_bf16(N, scale=0.5, seed=N + 4).to(DEV)
        res = fo.rand_bf16(64, N, seed=N + K + 6)
        tiles = N // 32
        for M in MS:
            rows = _rows(M)
            x_std = x[:M].contiguous().to(DEV)
            x_fr = fo.to_frag(x[:M], rows=rows, fill=float("nan")).to(DEV)
            parts = fo.synthetic_partials(x[:M], 7, seed=M, rows=rows).to(DEV)
            r_fr0 = fo.to_frag(res[:M], rows=rows, fill=3.0).to(DEV)
            r_std0 = res[:M].contiguous().to(DEV)
            for ks in KSPLIT:
                for xlds, yfrag, mode in _plain_variants(M, ks):
                    tag = (M, N, K, ks, xlds, yfrag, mode)
                    got = []
                    for pk in (p8, p16):
                        kw = dict(ks=ks, depth=1, xlds=xlds, yfrag=yfrag)
                        if xlds == 2:
                            kw.update(K=K, M_frag=M)
                        xin = x_fr if xlds == 2 else x_std
                        sq = torch.full((rows, tiles), float("nan"),
                                        device=DEV)
                        if mode == "res":
                            r = (r_fr0 if yfrag else r_std0).clone()
                            y = hip.linear_packed(xin, pk, None, N, res=r,
                                                  sq_out=sq, y=r, **kw)
                            got.append((_bits(y), sq[:M].clone()))
                            continue
                        if mode == "rstd":
                            kw.update(rstd=parts, rstd_nt=7, inv_h=1.0 / K,
                                      eps=fo.EPS)
                        y = hip.linear_packed(
                            xin, pk, None if mode == "none" else bias, N,
                            **kw)
                        live = fo.from_frag(y, M, N) if yfrag else y[:M]
                        got.append((_bits(live.contiguous()), None))
                    assert torch.equal(got[0][0], got[1][0]), \
                        (tag, int((got[0][0] != got[1][0]).sum()))
                    if mode == "res":
                        assert torch.equal(got[0][1], got[1][1]), tag
                    n_run += 1
    print(f"[w8] bits linear_packed K={K}: {n_run} combinations")
    assert n_run == 513          # every accepted combination really ran


@pytest.mark.parametrize("K", KS)
def test_bits_linear_gu(K):
    hip = _hip()
    for F in (16, 48):
        w = w8.normal(2 * F, K, seed=F + K)
        p8, p16, _ = _both_packs(hip, w, "gu")
        x = fo.rand_bf16(64, K, seed=K + F)
        for M in MS:
            rows = _rows(M)
            x_std = x[:M].contiguous().to(DEV)
            x_fr = fo.to_frag(x[:M], rows=rows, fill=float("nan")).to(DEV)
            parts = fo.synthetic_partials(x[:M], 7, seed=M, rows=rows).to(DEV)
            for frag, yfrag, nt in ((0, 0, 0), (0, 0, 7), (1, 0, 0),
                                    (1, 1, 7), (1, 1, 0), (0, 1, 7)):
                if M > 32 and not frag and (nt or yfrag):
                    continue             # fusion needs the frag path at MT2
                outs = []
                for pk in (p8, p16):
                    act = hip.linear_gu(
                        x_fr if frag else x_std, pk, 2 * F,
                        rstd=parts if nt else None, rstd_nt=nt,
                        inv_h=1.0 / K, eps=fo.EPS, yfrag=yfrag,
                        **(dict(K=K, M_frag=M) if frag else {}))
                    live = fo.from_frag(act, M, F) if yfrag else act[:M]
                    outs.append(_bits(live.contiguous()))
                assert torch.equal(outs[0], outs[1]), (M, F, K, frag, yfrag,
                                                       nt)


def _pool(nkl, M, seed):
    """72 shuffled slots, shuffled pages, sentinel bit patterns in every
    layer; rows alternate positions 0 and 17 (second page, offset 1)."""
    g = torch.Generator().manual_seed(seed)
    n_slots = 72
    slots = torch.randperm(n_slots, generator=g)[:M].int()
    ptab = torch.randperm(n_slots * 8, generator=g).int().reshape(n_slots, 8)
    pos = (torch.arange(M) % 2 * 17).int()
    kv = PagedKVCache(3, nkl, 128, page_size=16, n_pages=n_slots * 8,
                      max_slots=n_slots, max_ctx=fo.QKV_CTX, device=DEV,
                      dtype=torch.bfloat16)
    kv.page_table.copy_(ptab)
    k0 = tfe._sentinel(kv.k_pool.numel(), seed).reshape(kv.k_pool.shape)
    v0 = tfe._sentinel(kv.k_pool.numel(), seed + 1).reshape(kv.k_pool.shape)
    return kv, k0, v0, slots, pos, ptab


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("nl,nkl", [(4, 2), (7, 1)])
def test_bits_linear_qkv_rope(nl, nkl, K):
    hip = _hip()
    N = (nl + 2 * nkl) * 128
    w = w8.normal(N, K, seed=nl + K)
    p8, p16, _ = _both_packs(hip, w, "qkv", nl, nkl)
    order = torch.tensor(hip.qkv_rope_order(nl, nkl))
    bias_rp = fo.rand_bf16(N, scale=0.5, seed=N)[order].contiguous().to(DEV)
    cos, sin = (t.to(DEV) for t in fo.rope_tables(fo.QKV_CTX))
    x = fo.rand_bf16(64, K, seed=K + nl)
    for M in MS:
        rows = _rows(M)
        kv, k0, v0, slots, pos, ptab = _pool(nkl, M, seed=M + nl)
        parts = fo.synthetic_partials(x[:M], 7, seed=M, rows=rows).to(DEV)
        for frag in ((1,) if M > 32 else (0, 1)):
            xin = (fo.to_frag(x[:M], rows=rows, fill=float("nan")) if frag
                   else x[:M].contiguous()).to(DEV)
            outs = []
            for pk in (p8, p16):
                kv.k_pool.copy_(k0)
                kv.v_pool.copy_(v0)
                y = hip.linear_qkv_rope(
                    xin, pk, N, bias_rp, kv, 1, pos.to(DEV), slots.to(DEV),
                    cos, sin, nl, nkl, parts, 7, 1.0 / K, fo.EPS,
                    **(dict(K=K, M_real=M) if frag else {}))
                tfe._check_pools(kv, k0, v0, ptab, slots, pos, 1)
                outs.append((_bits(y[:, :nl * 128].contiguous()).cpu(),
                             _bits(kv.k_pool).cpu(), _bits(kv.v_pool).cpu()))
            for a, b, name in zip(outs[0], outs[1], ("q", "K pool", "V pool")):
                assert torch.equal(a, b), (name, nl, nkl, K, M, frag)


# ---------------------------------------------------------------------------
# exact


def _exact(t):
    """The oracle value is its own bf16 rounding."""
    assert torch.equal(t.bfloat16().double(), t)
    return t.bfloat16().to(DEV)


@pytest.mark.parametrize("K", [704, 3584])
def test_exact_scaled_rows(K):
    hip = _hip()
    for N in (96, 1024):
        w = w8.ternary_scaled(N, K, seed=N + K)
        p8, _, dq = _both_packs(hip, w)
        assert torch.equal(dq, w)
        mul = w8.scales(torch.arange(N, dtype=torch.int32) % 7 - 3)
        x = fo.ternary(64, K, seed=K + 1)
        # bias and residual carry their column's scale, so every result is
        # (integer <= 256) * 2^j: exact in bf16
        bias = (fo.int_bf16(N, lim=50, seed=N + 3).float() * mul).bfloat16()
        res = (fo.int_bf16(64, N, lim=100, seed=N + 5).float()
               * mul).bfloat16()
        for M in MS:
            rows = _rows(M)
            x_std = x[:M].contiguous().to(DEV)
            x_fr = fo.to_frag(x[:M], rows=rows, fill=float("nan")).to(DEV)
            yb = fo.gemm_oracle(x[:M], dq, bias=bias)[0]
            yr, sq, _, _ = fo.gemm_oracle(x[:M], dq, res=res[:M])
            assert float((yb / mul.double()).abs().max()) <= 256
            assert float((yr / mul.double()).abs().max()) <= 256
            want_b, want_r = _exact(yb), _exact(yr)
            for ks in KSPLIT:
                tag = (M, N, K, ks)
                if M <= 32:
                    y = hip.linear_packed(x_std, p8, bias.to(DEV), N, ks=ks,
                                          depth=1, xlds=0)
                    assert torch.equal(y, want_b), tag
                y = hip.linear_packed(x_fr, p8, bias.to(DEV), N, ks=ks,
                                      depth=1, xlds=2, K=K, M_frag=M)
                assert torch.equal(y[:M], want_b), tag
                r = fo.to_frag(res[:M], rows=rows).to(DEV)
                sq_out = torch.full((rows, N // 32), float("nan"),
                                    device=DEV)
                hip.linear_packed(x_fr, p8, None, N, ks=ks, depth=1, xlds=2,
                                  res=r, sq_out=sq_out, y=r, yfrag=1, K=K,
                                  M_frag=M)
                assert torch.equal(fo.from_frag(r, M, N), want_r), tag
                fo.assert_sq_close(sq_out[:M], sq, str(tag))


@pytest.mark.parametrize("nl,nkl,M,frag", [(4, 2, 64, 1), (7, 1, 33, 1),
                                           (4, 2, 5, 0)])
def test_exact_qkv_pair_order(nl, nkl, M, frag):
    """Position 0 (cos = 1, sin = 0): the pair-ordered scale vector, the
    pack and the pool addressing without arithmetic."""
    hip = _hip()
    K = 704
    N = (nl + 2 * nkl) * 128
    w = w8.ternary_scaled(N, K, seed=N)
    p8, _, dq = _both_packs(hip, w, "qkv", nl, nkl)
    assert torch.equal(dq, w)
    x = fo.ternary(M, K, seed=M)
    kv, k0, v0, slots, _, ptab = _pool(nkl, M, seed=nl)
    kv.k_pool.copy_(k0)
    kv.v_pool.copy_(v0)
    pos = torch.zeros(M, dtype=torch.int32)
    cos, sin = fo.rope_tables(fo.QKV_CTX)
    q, k, v = fo.qkv_oracle(x, dq, nl, nkl, pos, cos, sin)
    xin = fo.to_frag(x, rows=_rows(M), fill=float("nan")) if frag else x
    y = hip.linear_qkv_rope(
        xin.to(DEV), p8, N, None, kv, 1, pos.to(DEV), slots.to(DEV),
        cos.to(DEV), sin.to(DEV), nl, nkl, None, 0, 0.0, 0.0,
        **(dict(K=K, M_real=M) if frag else {}))
    assert torch.equal(y[:, :nl * 128].reshape(M, nl, 128), _exact(q))
    kg, vg = tfe._check_pools(kv, k0, v0, ptab, slots, pos, 1)
    assert torch.equal(kg.to(DEV), _exact(k))
    assert torch.equal(vg.to(DEV), _exact(v))


# ---------------------------------------------------------------------------
# real


@pytest.mark.parametrize("case", [c for c in fo.RSTD_CASES
                                  if c[3] in (7, 112)], ids=str)
def test_real_rstd_gemm(case):
    hip = _hip()
    M, N, K, nt, mode = case
    x, w, bias, res, parts = fo.rstd_inputs(M, N, K, nt)
    p8, _, dq = _both_packs(hip, w)
    inv_h, eps = 1.0 / K, fo.EPS
    rows = _rows(M)
    xin = fo.to_frag(x, rows=rows, fill=float("nan")).to(DEV)
    kw = dict(K=K, M_frag=M, xlds=2, depth=1, rstd=parts.to(DEV),
              rstd_nt=nt, inv_h=inv_h, eps=eps)
    if mode == "bias":
        truth = fo.gemm_oracle(x, dq, parts, inv_h, eps, bias)[0]
        y = hip.linear_packed(xin, p8, bias.to(DEV), N, **kw)
        worst = fo.assert_bf16_close(y[:M], truth, str(case))
    else:
        truth, sq, _, _ = fo.gemm_oracle(x, dq, parts, inv_h, eps, None, res)
        r = fo.to_frag(res, rows=rows, fill=float("nan")).to(DEV)
        sq_out = torch.full((rows, N // 32), float("nan"), device=DEV)
        hip.linear_packed(xin, p8, None, N, res=r, sq_out=sq_out, y=r,
                          yfrag=1, **kw)
        worst = fo.assert_bf16_close(fo.from_frag(r, M, N), truth, str(case))
        fo.assert_sq_close(sq_out[:M], sq, str(case))
    print(f"[w8] real rstd_gemm {case}: worst normalised error {worst:.3f}")


@pytest.mark.parametrize("case", fo.GU_CASES, ids=str)
def test_real_linear_gu(case):
    hip = _hip()
    M, F, K, nt, frag, yfrag, gscale = case
    x, w, parts = fo.gu_inputs(M, F, K, nt, gscale)
    p8, _, dq = _both_packs(hip, w, "gu")
    truth = fo.gu_oracle(x, dq, parts, 1.0 / K, fo.EPS)
    xin = (fo.to_frag(x, rows=_rows(M), fill=float("nan")) if frag
           else x).to(DEV)
    act = hip.linear_gu(
        xin, p8, 2 * F, rstd=parts.to(DEV) if nt else None, rstd_nt=nt,
        inv_h=1.0 / K, eps=fo.EPS, yfrag=yfrag,
        **(dict(K=K, M_frag=M) if frag else {}))
    got = fo.from_frag(act, M, F) if yfrag else act[:M]
    worst = fo.assert_bf16_close(got, truth, str(case))
    print(f"[w8] real linear_gu {case}: worst normalised error {worst:.3f}")


@pytest.mark.parametrize("case", fo.QKV_CASES, ids=str)
def test_real_qkv_rope(case):
    hip = _hip()
    nl, nkl, K, M, use_bias, frag, nt = case
    N = (nl + 2 * nkl) * 128
    x, w, bias, parts, slots, pos, ptab = fo.qkv_inputs(nl, nkl, K, M, nt)
    p8, _, dq = _both_packs(hip, w, "qkv", nl, nkl)
    cos, sin = fo.rope_tables(fo.QKV_CTX)
    q, k, v = fo.qkv_oracle(x, dq, nl, nkl, pos, cos, sin, parts, 1.0 / K,
                            fo.EPS, bias if use_bias else None)
    kv, k0, v0 = tfe._qkv_cache(nkl, ptab, seed=nl + K)
    order = torch.tensor(hip.qkv_rope_order(nl, nkl))
    xin = fo.to_frag(x, rows=_rows(M), fill=float("nan")) if frag else x
    y = hip.linear_qkv_rope(
        xin.to(DEV), p8, N,
        bias[order].contiguous().to(DEV) if use_bias else None, kv, 1,
        pos.to(DEV), slots.to(DEV), cos.to(DEV), sin.to(DEV), nl, nkl,
        parts.to(DEV) if nt else None, nt, 1.0 / K, fo.EPS,
        **(dict(K=K, M_real=M) if frag else {}))
    worst = fo.assert_bf16_close(y[:, :nl * 128].reshape(M, nl, 128), q,
                                 f"q {case}")
    kg, vg = tfe._check_pools(kv, k0, v0, ptab, slots, pos, 1)
    worst = max(worst, fo.assert_bf16_close(kg, k, f"k {case}"),
                fo.assert_bf16_close(vg, v, f"v {case}"))
    print(f"[w8] real qkv_rope {case}: worst normalised error {worst:.3f}")


# ---------------------------------------------------------------------------
# wrapper contract


def test_wrapper_contract_fp8_depth():
    """An fp8 pack streams at depth == 1 only: depth == 2 raises before
    anything is launched, for every xlds; depth == 1 computes."""
    hip = _hip()
    M, N, K = 7, 96, 704
    w = w8.normal(N, K, seed=1)
    p8, _, dq = _both_packs(hip, w)
    x = fo.rand_bf16(M, K, seed=2)
    x_fr = fo.to_frag(x, rows=32).to(DEV)
    canary = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    for xlds in (0, 1, 2):
        xin, kw = (x_fr, dict(K=K, M_frag=M)) if xlds == 2 \
            else (x.to(DEV), {})
        with pytest.raises(ValueError):
            hip.linear_packed(xin, p8, None, N, ks=1, depth=2, xlds=xlds,
                              y=canary, **kw)
        torch.cuda.synchronize()
        assert bool((canary == 7.0).all())
        y = hip.linear_packed(xin, p8, None, N, ks=1, depth=1, xlds=xlds,
                              **kw)
        fo.assert_bf16_close(y[:M], fo.gemm_oracle(x, dq)[0], f"xlds {xlds}")
