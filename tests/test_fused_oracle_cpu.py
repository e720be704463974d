"""Soundness of the fused-chain test helpers (tests/fused_oracle.py): the
frag-layout index arithmetic, the weight packs, and the tolerances.  An
"ideal kernel" (fp32 throughout, one bf16 rounding at the end) must sit
inside assert_bf16_close at every shape the GPU tests use, so a GPU
failure there means the kernel, not the yardstick.  No GPU needed.
"""
import pytest
import torch

import fused_oracle as fo
from ollamamq_amd.ops import hip


def _frag_off(m, kcol):
    """Scalar transcription of frag_off() in csrc/kernels/common.cuh."""
    b, j, h = kcol >> 6, (kcol >> 4) & 3, (kcol >> 3) & 1
    return (((b * 4 + j) * 64) + h * 32 + m) * 8 + (kcol & 7)


def test_frag_helpers_match_scalar_formula():
    M, K = 64, 128
    x = torch.arange(M * K, dtype=torch.float32).reshape(M, K)
    flat = fo.to_frag(x, rows=64)
    assert flat.numel() == 64 * K
    for m in range(M):
        for k in range(K):
            off = (m >> 5) * 32 * K + _frag_off(m & 31, k)
            assert flat[off] == x[m, k], (m, k)
    assert torch.equal(fo.from_frag(flat, M, K), x)
    # partial fill: dead rows keep the fill value, live rows round-trip
    part = fo.to_frag(x[:33], rows=64, fill=-1.0)
    assert torch.equal(fo.from_frag(part, 33, K), x[:33])
    assert int((part == -1.0).sum()) == 31 * K
    assert torch.equal(fo.from_frag(fo.to_frag(x[:7], rows=32), 7, K), x[:7])


def test_pack_weight_matches_documented_formula():
    N, K = 64, 128
    NB = K // 64
    w = torch.arange(N * K, dtype=torch.float32).reshape(N, K).bfloat16()
    w = (w.float() % 251).bfloat16()          # exact in bf16, non-trivial
    pk = hip.pack_weight(w)
    for n in range(N):
        for k in range(K):
            t, r = n // 32, n % 32
            b, j, h, e = k // 64, (k // 16) % 4, (k // 8) % 2, k % 8
            unit = ((t * NB + b) * 4 + j) * 64 + (h * 32 + r)
            assert pk[unit * 8 + e] == w[n, k], (n, k)


def test_pack_weight_gu_matches_documented_formula():
    F, K = 48, 128
    NB = K // 64
    w = (torch.arange(2 * F * K, dtype=torch.float32) % 251) \
        .reshape(2 * F, K).bfloat16()
    pk = hip.pack_weight_gu(w)
    plain = hip.pack_weight(w)
    assert pk.numel() == plain.numel()
    # tile t: rows 0..15 = gate f = t*16 + r, rows 16..31 = up of the same f
    for t in range(F // 16):
        for r in range(32):
            src = t * 16 + r if r < 16 else F + t * 16 + (r - 16)
            for k in range(K):
                b, j, h, e = k // 64, (k // 16) % 4, (k // 8) % 2, k % 8
                unit = ((t * NB + b) * 4 + j) * 64 + (h * 32 + r)
                assert pk[unit * 8 + e] == w[src, k], (t, r, k)


@pytest.mark.parametrize("nl,nkl", [(1, 1), (4, 2), (7, 1), (3, 3)])
def test_qkv_rope_order(nl, nkl):
    order = hip.qkv_rope_order(nl, nkl)
    N = (nl + 2 * nkl) * 128
    assert sorted(order) == list(range(N))
    # scalar transcription: packed row p of head hd, tile quarter d0
    for p, src in enumerate(order):
        if p < (nl + nkl) * 128:
            hd, within = p // 128, p % 128
            d0, c = (within // 32) * 16, within % 32
            want = hd * 128 + d0 + (c if c < 16 else 64 + c - 16)
        else:
            want = p
        assert src == want, (p, src, want)
    # every 32-row q/k tile: 16 dims then the same dims + 64, one head
    for t in range((nl + nkl) * 4):
        tile = order[t * 32:(t + 1) * 32]
        assert tile[16:] == [d + 64 for d in tile[:16]]
        assert tile[:16] == list(range(tile[0], tile[0] + 16))
        assert tile[0] // 128 == tile[31] // 128 == t // 4
        assert tile[0] % 128 == (t % 4) * 16
    # the pack is the plain pack of the row-permuted weight
    w = fo.rand_bf16(N, 64, seed=nl)
    assert torch.equal(hip.pack_weight_qkv_rope(w, nl, nkl),
                       hip.pack_weight(w[torch.tensor(order)].contiguous()))


def test_partials_helpers():
    x = fo.rand_bf16(33, 704, seed=1)
    true = (x.double() ** 2).sum(1)
    for nt in fo.RSTD_NT:
        p = fo.synthetic_partials(x, nt, seed=nt, rows=64)
        assert p.shape == (64, nt) and p.dtype == torch.float32
        assert (p[:33] > 0).all() and torch.isnan(p[33:]).all()
        torch.testing.assert_close(p[:33].double().sum(1), true,
                                   rtol=1e-6, atol=0)
        u = fo.unit_partials(33, nt, seed=nt, rows=64)
        assert torch.isnan(u[33:]).all()
        # exact in fp32 in any order: forwards, backwards, strided by 8/16
        assert torch.equal(u[:33].sum(1), torch.ones(33))
        assert torch.equal(u[:33].flip(1).cumsum(1)[:, -1], torch.ones(33))
        assert float(fo.rstd_from_parts(u[:33], 1.0, 0.0).sub(1).abs()
                     .max()) == 0.0


def test_tolerance_helpers_reject_real_errors():
    t = fo.rand_bf16(40, 96, seed=2).double() * 10
    assert fo.assert_bf16_close(t.bfloat16(), t) <= 0.51
    bad = t.clone()
    bad[37, 5] += 2.0 ** -6 * t[37, 5].abs() + 0.2   # two ulps + abs term
    with pytest.raises(AssertionError):
        fo.assert_bf16_close(bad, t)
    with pytest.raises(AssertionError):
        fo.assert_bf16_close(torch.full_like(t, float("nan")), t)
    sq = t.pow(2).reshape(40, 3, 32).sum(-1)
    fo.assert_sq_close(sq.float(), sq)
    bad = sq.clone()
    bad[39, 2] *= 1.004
    with pytest.raises(AssertionError):
        fo.assert_sq_close(bad, sq)


# ---------------------------------------------------------------------------
# the "ideal kernel": same formula, fp32 throughout, one bf16 rounding


def _ideal_gemm(x, w, parts=None, inv_h=0.0, eps=0.0, bias=None, res=None):
    acc = x.float() @ w.float().t()
    if parts is not None:
        rstd = torch.rsqrt(parts[:x.shape[0]].sum(1) * inv_h + eps)
        acc = acc * rstd.unsqueeze(1)
    if bias is not None:
        acc = acc + bias.float()
    if res is not None:
        acc = acc + res.float()
    M, N = acc.shape
    return acc, (acc * acc).reshape(M, N // 32, 32).sum(-1)


@pytest.mark.parametrize("case", fo.RSTD_CASES, ids=str)
def test_ideal_kernel_rstd_gemm_inside_tolerance(case):
    M, N, K, nt, mode = case
    x, w, bias, res, parts = fo.rstd_inputs(M, N, K, nt)
    b, r = (bias, None) if mode == "bias" else (None, res)
    truth, sq, rstd, _ = fo.gemm_oracle(x, w, parts, 1.0 / K, fo.EPS, b, r)
    assert float((rstd - 1).abs().max()) < 0.2      # unit-variance rows
    y, ysq = _ideal_gemm(x, w, parts, 1.0 / K, fo.EPS, b, r)
    fo.assert_bf16_close(y.bfloat16(), truth)
    fo.assert_sq_close(ysq, sq)
    # the plain formula on the same inputs
    fo.assert_bf16_close(_ideal_gemm(x, w)[0].bfloat16(),
                         fo.gemm_oracle(x, w)[0])


@pytest.mark.parametrize("case", fo.GU_CASES, ids=str)
def test_ideal_kernel_swiglu_inside_tolerance(case):
    M, F, K, nt, _, _, gscale = case
    x, w, parts = fo.gu_inputs(M, F, K, nt, gscale)
    truth = fo.gu_oracle(x, w, parts, 1.0 / K, fo.EPS)
    gu = _ideal_gemm(x, w, parts, 1.0 / K, fo.EPS)[0]
    g, u = gu[:, :F], gu[:, F:]
    if gscale != 1.0:
        assert float(g.abs().max()) > 80.0
    act = (g / (1.0 + torch.exp(-g))) * u
    fo.assert_bf16_close(act.bfloat16(), truth)


@pytest.mark.parametrize("case", fo.QKV_CASES, ids=str)
def test_ideal_kernel_qkv_rope_inside_tolerance(case):
    nl, nkl, K, M, use_bias, _, nt = case
    x, w, bias, parts, slots, pos, ptab = fo.qkv_inputs(nl, nkl, K, M, nt)
    cos, sin = fo.rope_tables(fo.QKV_CTX)
    b = bias if use_bias else None
    q, k, v = fo.qkv_oracle(x, w, nl, nkl, pos, cos, sin, parts, 1.0 / K,
                            fo.EPS, b)
    y = _ideal_gemm(x, w, parts, 1.0 / K, fo.EPS, b)[0]
    c = cos[pos.long()].unsqueeze(1)
    s = sin[pos.long()].unsqueeze(1)

    def rot(t):
        lo, hi = t[..., :64], t[..., 64:]
        return torch.cat([lo * c - hi * s, hi * c + lo * s], -1)

    yq = y[:, :nl * 128].reshape(M, nl, 128)
    yk = y[:, nl * 128:(nl + nkl) * 128].reshape(M, nkl, 128)
    yv = y[:, (nl + nkl) * 128:].reshape(M, nkl, 128)
    fo.assert_bf16_close(rot(yq).bfloat16(), q)
    fo.assert_bf16_close(rot(yk).bfloat16(), k)
    fo.assert_bf16_close(yv.bfloat16(), v)
    # the addressing inputs are what the GPU test relies on
    assert len(set(zip(slots.tolist(), pos.tolist()))) == M
    assert {0, 15, 16, 31, 32}.issubset(set(pos.tolist()))
    assert sorted(ptab.reshape(-1).tolist()) == list(range(ptab.numel()))
    assert slots.tolist() != sorted(slots.tolist())
    _, pages, offs = fo.paged_coords(ptab, slots, pos, 16, 1)
    assert len(set(zip(pages.tolist(), offs.tolist()))) == M


def test_position_zero_rope_is_identity():
    cos, sin = fo.rope_tables(4)
    assert torch.equal(cos[0], torch.ones(64))
    assert torch.equal(sin[0], torch.zeros(64))
    t = fo.int_bf16(5, 3, 128, lim=100, seed=4).double()
    assert torch.equal(fo.rope_oracle(t, torch.zeros(5, dtype=torch.int32),
                                      cos, sin), t)


@pytest.mark.parametrize("K", fo.TIER_A_K)
def test_tier_a_inputs_are_exact(K):
    """Integer tier: every result is an integer <= 256 (exact in bf16) and
    every sum-of-squares partial an integer < 2^24 (exact in fp32 in any
    summation order)."""
    for N in fo.TIER_A_N:
        x, w, bias, res = fo.tier_a_inputs(N, K)
        assert set(x.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert 0.4 < float((w != 0).float().mean()) < 0.6
        for b, r in ((None, None), (bias, None), (None, res), (bias, res)):
            y, sq, _, _ = fo.gemm_oracle(x, w, bias=b, res=r)
            assert torch.equal(y, y.round())
            assert float(y.abs().max()) <= 256
            assert torch.equal(y.bfloat16().double(), y)
            assert float(sq.max()) < 2 ** 24
            assert torch.equal(sq.float().double(), sq)
