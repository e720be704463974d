"""fp64 oracles, frag-layout helpers and tolerances for the fused decode
chain (tests/test_fused_oracle_cpu.py proves them on the CPU,
tests/test_fused_epilogues_gpu.py applies them to the HIP kernels).

Everything here is plain torch on the CPU.  The oracles take the SAME
bf16 inputs the kernels see, upcast to double, so the only legitimate
difference between a kernel and its oracle is fp32 accumulation order
and the single bf16 rounding of the output.
"""
import functools

import torch

EPS = 1e-5

# ---------------------------------------------------------------------------
# frag layout: element (m, k), k = b*64 + j*16 + h*8 + e, lives at 16-byte
# unit ((b*4 + j)*64 + h*32 + (m % 32)), element e; rows 32..63 sit in a
# second block at +32*K elements.


@functools.lru_cache(maxsize=64)
def _frag_index_on(rows, K, device):
    return frag_index(rows, K).to(device)


def frag_index(rows, K):
    """[rows, K] int64 flat element offsets of the frag layout."""
    m = torch.arange(rows).unsqueeze(1)
    k = torch.arange(K).unsqueeze(0)
    b, j, h, e = k >> 6, (k >> 4) & 3, (k >> 3) & 1, k & 7
    unit = (b * 4 + j) * 64 + h * 32 + (m % 32)
    return unit * 8 + e + (m // 32) * 32 * K


def to_frag(x, rows=32, fill=0.0):
    """[M, K] -> flat frag buffer of `rows` (32 or 64) rows; rows >= M
    hold `fill`."""
    M, K = x.shape
    assert rows in (32, 64) and M <= rows and K % 16 == 0
    flat = torch.full((rows * K,), fill, dtype=x.dtype, device=x.device)
    idx = _frag_index_on(M, K, str(x.device))
    flat[idx.reshape(-1)] = x.reshape(-1)
    return flat


def from_frag(flat, M, K):
    """Read rows 0..M-1 of a flat frag buffer back to [M, K]."""
    flat = flat.reshape(-1)
    return flat[_frag_index_on(M, K, str(flat.device))]


# ---------------------------------------------------------------------------
# oracles


def rstd_from_parts(parts, inv_h, eps):
    """rstd[m] = rsqrt(sum_t parts[m, t] * inv_h + eps) in fp64."""
    return torch.rsqrt(parts.double().sum(1) * inv_h + eps)


def gemm_oracle(x, w, parts=None, inv_h=0.0, eps=0.0, bias=None, res=None):
    """y = ((x @ w^T) * rstd + bias) + res in fp64.

    Returns (y, sq, rstd, pre): the full result, the per-32-column
    sum-of-squares partials [M, N/32] of the unrounded y, the rstd vector
    (None without parts) and the result before the residual add."""
    acc = x.double() @ w.double().t()
    rstd = None
    if parts is not None:
        rstd = rstd_from_parts(parts[:x.shape[0]], inv_h, eps)
        acc = acc * rstd.unsqueeze(1)
    if bias is not None:
        acc = acc + bias.double()
    pre = acc
    y = acc + res.double() if res is not None else acc
    M, N = y.shape
    sq = (y * y).reshape(M, N // 32, 32).sum(-1)
    return y, sq, rstd, pre


def swiglu_oracle(gu):
    """silu(gate) * up on a [M, 2F] = [gate | up] fp64 tensor."""
    F = gu.shape[1] // 2
    g, u = gu[:, :F], gu[:, F:]
    return g * torch.sigmoid(g) * u


def gu_oracle(x, w, parts=None, inv_h=0.0, eps=0.0):
    gu = gemm_oracle(x, w, parts, inv_h, eps)[0]
    return swiglu_oracle(gu)


def rope_oracle(t, positions, cos, sin):
    """NeoX half rotation of t [M, heads, 128] (fp64) with the fp32
    cos/sin tables [ctx, 64]."""
    c = cos[positions.long()].double().unsqueeze(1)
    s = sin[positions.long()].double().unsqueeze(1)
    lo, hi = t[..., :64], t[..., 64:]
    return torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1)


def paged_coords(page_table, slots, positions, page_size, layer):
    """(layer, page[M], offset[M]) of each row's KV entry; the heads span
    dim 2 of the pool: pool[layer, page, head, offset]."""
    pages = page_table[slots.long(), (positions // page_size).long()].long()
    return layer, pages, (positions % page_size).long()


def qkv_oracle(x, w, nl, nkl, positions, cos, sin, parts=None, inv_h=0.0,
               eps=0.0, bias=None):
    """(q, k, v) fp64: rope(q) [M, nl, 128], rope(k) and v [M, nkl, 128]."""
    y = gemm_oracle(x, w, parts, inv_h, eps, bias)[0]
    M = y.shape[0]
    q = y[:, :nl * 128].reshape(M, nl, 128)
    k = y[:, nl * 128:(nl + nkl) * 128].reshape(M, nkl, 128)
    v = y[:, (nl + nkl) * 128:].reshape(M, nkl, 128)
    return (rope_oracle(q, positions, cos, sin),
            rope_oracle(k, positions, cos, sin), v)


def rope_tables(ctx, theta=10000.0):
    ang = torch.outer(torch.arange(ctx, dtype=torch.float32),
                      1.0 / theta ** (torch.arange(0, 128, 2).float() / 128))
    return ang.cos(), ang.sin()


# ---------------------------------------------------------------------------
# inputs


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rand_bf16(*shape, scale=1.0, seed=0):
    return (torch.randn(*shape, generator=_gen(seed)) * scale).bfloat16()


def ternary(*shape, seed=0):
    """{-1, 0, +1} at density 1/2, bf16."""
    g = _gen(seed)
    mag = torch.randint(0, 2, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sign).bfloat16()


def int_bf16(*shape, lim, seed=0):
    return torch.randint(-lim, lim + 1, shape, generator=_gen(seed)).bfloat16()


def synthetic_partials(x, nt, seed=0, rows=None):
    """Split each row's true sum of squares into nt positive fp32
    partials, m-major [rows, nt]; rows >= M are NaN (the kernels read but
    never use them)."""
    M = x.shape[0]
    true = (x.double() ** 2).sum(1)
    wgt = torch.rand(M, nt, generator=_gen(seed), dtype=torch.float64) + 0.1
    wgt = wgt / wgt.sum(1, keepdim=True)
    out = torch.full((rows or M, nt), float("nan"), dtype=torch.float32)
    out[:M] = (true.unsqueeze(1) * wgt).float()
    return out


def unit_partials(M, nt, seed=0, rows=None):
    """Dyadic partials (multiples of 1/64) that sum to exactly 1 per row
    in any fp32 order: with inv_h = 1 and eps = 0 the rstd is exactly 1,
    so the integer tier stays exact through the fold.  Dead rows NaN."""
    g = _gen(seed)
    pick = torch.randint(0, nt, (M, 64), generator=g)
    cnt = torch.zeros(M, nt).scatter_add_(1, pick, torch.ones(M, 64))
    out = torch.full((rows or M, nt), float("nan"), dtype=torch.float32)
    out[:M] = cnt / 64.0
    return out


# ---------------------------------------------------------------------------
# tolerances


def assert_bf16_close(got, truth, what=""):
    """Per element |got - truth| <= 2^-7 |truth| + 2^-8 rms(truth).

    One bf16 ulp relative (a correctly rounded fp32 result needs half of
    it; the other half covers fp32 summation order moving a value across a
    rounding boundary) plus a 2^-8 error at the tensor's typical magnitude
    for elements that are small through cancellation.  Returns the worst
    error normalised by that budget."""
    g = got.detach().double().cpu()
    t = truth.detach().double().cpu()
    assert g.shape == t.shape, f"{what}: shape {g.shape} vs {t.shape}"
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    rms = t.pow(2).mean().sqrt()
    budget = t.abs() * 2.0 ** -7 + rms * 2.0 ** -8
    err = (g - t).abs()
    if float(rms) == 0.0:
        assert float(err.max()) == 0.0, f"{what}: nonzero vs all-zero truth"
        return 0.0
    worst = float((err / budget).max())
    assert worst <= 1.0, (
        f"{what}: worst normalised error {worst:.3f} at "
        f"{tuple(int(i) for i in (err / budget).argmax().unsqueeze(0))} "
        f"(max abs err {float(err.max()):.4g}, rms {float(rms):.4g})")
    return worst


def assert_sq_close(got, truth, what=""):
    """Sum-of-squares partials: rtol 2^-10 plus atol 2^-10 x the mean
    partial (fp32 accumulation noise is <= K * 2^-24; the partials are
    taken before bf16 rounding, so nothing larger is legitimate)."""
    g = got.detach().double().cpu()
    t = truth.detach().double().cpu()
    assert g.shape == t.shape, f"{what}: shape {g.shape} vs {t.shape}"
    assert torch.isfinite(g).all(), f"{what}: non-finite partials"
    budget = t.abs() * 2.0 ** -10 + t.mean() * 2.0 ** -10
    err = (g - t).abs()
    worst = float((err / budget).max())
    assert worst <= 1.0, f"{what}: sq partial error {worst:.3f} x budget"
    return worst


# ---------------------------------------------------------------------------
# the case lists shared by the CPU soundness tests and the GPU tests

TIER_A_K = (64, 256, 704, 1536, 3584)
TIER_A_M = (1, 7, 31, 32, 33, 47, 64)
TIER_A_N = (32, 96, 1024)
TIER_A_KS = (1, 2, 3, 8)
RSTD_NT = (1, 7, 16, 112)


def tier_a_inputs(N, K):
    """Integer-exact GEMM inputs: x [64, K], w [N, K], bias, res [64, N]."""
    return (ternary(64, K, seed=K + 1), ternary(N, K, seed=N * 7 + K),
            int_bf16(N, lim=50, seed=N + 3), int_bf16(64, N, lim=100,
                                                      seed=N + K + 5))


# (M, N, K, nt, mode): mode "bias" = rstd + bias, "res" = rstd + residual
# + sq_out.  M <= 32 runs MT=1 (fold width 16), M > 32 MT=2 (fold width 8).
RSTD_CASES = [(M, 96, 704, nt, mode)
              for nt in RSTD_NT for M in (31, 47)
              for mode in ("bias", "res")] + \
             [(32, 1024, 3584, 112, "res"), (64, 1024, 3584, 112, "res"),
              (7, 32, 64, 7, "bias"), (33, 32, 256, 16, "bias")]


def rstd_inputs(M, N, K, nt):
    x = rand_bf16(M, K, seed=M + K)
    w = rand_bf16(N, K, scale=K ** -0.5, seed=N + K + 1)
    bias = rand_bf16(N, scale=0.5, seed=N + 2)
    res = rand_bf16(M, N, seed=M + N + 3)
    parts = synthetic_partials(x, nt, seed=nt, rows=32 * ((M + 31) // 32))
    return x, w, bias, res, parts


# (M, F, K, rstd_nt (0 = off), frag input, yfrag, gate scale)
GU_CASES = [
    (7, 16, 256, 0, 0, 0, 1.0),
    (32, 48, 704, 7, 0, 0, 1.0),
    (31, 1024, 256, 16, 0, 1, 1.0),
    (1, 48, 256, 1, 1, 0, 1.0),
    (31, 16, 704, 112, 1, 1, 1.0),
    (33, 48, 704, 7, 1, 1, 1.0),
    (47, 1024, 256, 0, 1, 0, 1.0),
    (64, 1024, 3584, 112, 1, 1, 1.0),
    (64, 16, 256, 16, 1, 0, 1.0),
    (47, 48, 256, 0, 0, 0, 1.0),     # standard x at MT=2 (generic path)
    (32, 48, 704, 16, 0, 0, 40.0),   # gate pre-activations reach ~ +-100
    (64, 48, 704, 0, 1, 1, 40.0),
]


def gu_inputs(M, F, K, nt, gscale):
    x = rand_bf16(M, K, seed=M + F + K)
    w = rand_bf16(2 * F, K, scale=K ** -0.5, seed=F + K + 1)
    if gscale != 1.0:
        w = torch.cat([w[:F].float() * gscale, w[F:].float()]).bfloat16()
    parts = synthetic_partials(x, nt, seed=nt + 1,
                               rows=32 * ((M + 31) // 32)) if nt else None
    return x, w, parts


# (nl, nkl, K, M, bias, frag input, rstd_nt (0 = off))
QKV_CASES = [
    (2, 1, 256, 7, 0, 0, 0),
    (2, 1, 3584, 33, 1, 1, 112),
    (4, 2, 256, 32, 1, 0, 1),
    (4, 2, 3584, 64, 0, 1, 16),
    (7, 1, 256, 64, 1, 1, 7),
    (7, 1, 3584, 7, 0, 1, 1),
    (3, 3, 256, 33, 0, 1, 0),
    (3, 3, 3584, 31, 1, 0, 7),
]
QKV_CTX = 128          # 8 pages of 16 per slot
QKV_SLOTS = 24


def qkv_inputs(nl, nkl, K, M, nt, seed=0):
    """x, w [N, K], bias [N], rstd partials, slots [M], positions [M],
    page table [QKV_SLOTS, 8]: shuffled slot ids and page ids, positions
    over several pages with the page-boundary offsets 0, 15 and 16
    forced in, distinct (slot, position) per row."""
    N = (nl + 2 * nkl) * 128
    s = seed + nl * 100 + nkl * 10 + K + M
    x = rand_bf16(M, K, seed=s)
    w = rand_bf16(N, K, scale=K ** -0.5, seed=s + 1)
    bias = rand_bf16(N, scale=0.5, seed=s + 2)
    parts = synthetic_partials(x, nt, seed=s + 3,
                               rows=32 * ((M + 31) // 32)) if nt else None
    g = _gen(s + 4)
    forced = [((i * 7 + 5) % QKV_SLOTS) * QKV_CTX + p for i, p in
              enumerate([0, 15, 16, 31, 32, QKV_CTX - 1][:M])]
    perm = torch.randperm(QKV_SLOTS * QKV_CTX, generator=g).tolist()
    rest = [p for p in perm if p not in forced][:M - len(forced)]
    pairs = torch.tensor(forced + rest)
    assert pairs.unique().numel() == M
    slots = (pairs // QKV_CTX).int()
    pos = (pairs % QKV_CTX).int()
    n_pages = QKV_SLOTS * (QKV_CTX // 16)
    ptab = torch.randperm(n_pages, generator=g).int().reshape(QKV_SLOTS, -1)
    return x, w, bias, parts, slots, pos, ptab
