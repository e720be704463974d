"""fp64 oracles, a bit-exact emulation of the sampler's counter noise,
adversarial append pools, fp32 emulations and case lists for the
elementwise and sampler kernels of kernels.hip (tests/test_elem_oracle_cpu.py
proves them on the CPU, tests/test_elementwise_gpu.py and
tests/test_sampler_kernels_gpu.py apply them to k_rmsnorm_residual, k_rope,
k_kv_append, k_rope_append, k_swiglu, k_embed_gather, k_row_sumsq,
k_argmax* and k_gumbel_*).

Everything here is plain torch / numpy on the CPU.  The oracles take the
SAME bf16 inputs the kernels see, upcast to double, so the only legitimate
difference is fp32 arithmetic and the single bf16 rounding of the output.
swiglu_oracle, rope_oracle, paged_coords, rope_tables and the budgets come
from fused_oracle, the pool builder from attn_oracle.
"""
import functools

import numpy as np
import torch

import attn_oracle as ao
import fused_oracle as fo

D = 128
EPS = 1e-5


def assert_rows_close(got, truth, what=""):
    """fo.assert_bf16_close row by row (the rms of the budget is taken per
    row of the leading dim).  Returns the worst normalised error."""
    g = got.detach().cpu()
    assert g.shape == truth.shape, f"{what}: {g.shape} vs {truth.shape}"
    worst = 0.0
    for r in range(g.shape[0]):
        worst = max(worst, fo.assert_bf16_close(g[r], truth[r],
                                                f"{what} row {r}"))
    return worst


def bits(t):
    """bf16 tensor -> int16 view on the CPU: bit equality that also holds
    for NaN payloads."""
    return t.detach().cpu().contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# rmsnorm + residual

# every instantiation of k_rmsnorm_residual<VPT, EXACT>: <1,f> at 8 (one
# live thread), 512, 2040; <1,t> 2048; <2,f> 2056 (one-vector tail), 3584;
# <2,t> 4096; <4,f> 4104 (tail), 5120; <4,t> 8192; <8,f> 8200 (tail);
# <8,t> 16384
RMS_H = (8, 512, 2040, 2048, 2056, 3584, 4096, 4104, 5120, 8192, 8200, 16384)
RMS_T = (1, 5)
SPIKE = 64.0


def rms_inputs(T, H):
    """x, res [T, H] N(0,1) and w [H] around 1, bf16."""
    x = fo.rand_bf16(T, H, seed=3 * H + T)
    res = fo.rand_bf16(T, H, seed=3 * H + T + 1)
    w = (fo.rand_bf16(H, scale=0.5, seed=3 * H + 2).float() + 1.0).bfloat16()
    return x, res, w


def spike_positions(H):
    return sorted({p for p in (0, 7, 8, 2047, 2048, H - 8, H - 1)
                   if 0 <= p < H})


def spike_inputs(H, with_res):
    """One row per spike position: x + res is +-1 everywhere except SPIKE at
    that position; w uniform in [0.5, 1.5].  The spike holds 4096 of the
    row's H + 4095 sum of squares: the 16-byte vector that carries it
    missing from the reduction moves rstd by a factor sqrt((H + 4095) /
    (H - 8)), 23x at H = 16, 2.0x at H = 2048 and still 1.29x at
    H = 16384, against a budget of one bf16 ulp (0.8 %)."""
    pos = spike_positions(H)
    g = torch.Generator().manual_seed(7 * H + int(with_res))
    sign = (torch.randint(0, 2, (len(pos), H), generator=g) * 2 - 1).float()
    w = (torch.rand(H, generator=g) + 0.5).bfloat16()
    if with_res:
        x, res = sign * 2, -sign            # +-2 -+ 1 = +-1
        for r, p in enumerate(pos):
            x[r, p] = res[r, p] = SPIKE / 2
        return x.bfloat16(), res.bfloat16(), w
    x = sign
    for r, p in enumerate(pos):
        x[r, p] = SPIKE
    return x.bfloat16(), None, w


def res_out_exact(x, res):
    """What res_out must be bit for bit: the fp32 sum rounded once."""
    return x if res is None else (x.float() + res.float()).bfloat16()


def rmsnorm_oracle(x, res, w, eps=EPS):
    """y = (x + res) * rsqrt(mean((x + res)^2) + eps) * w in fp64, on the
    unrounded sum, as the kernel keeps it in registers."""
    h = x.double() if res is None else x.double() + res.double()
    rstd = torch.rsqrt(h.pow(2).mean(dim=1, keepdim=True) + eps)
    return h * rstd * w.double()


def emulate_rmsnorm(x, res, w, eps=EPS):
    """fp32 throughout, one bf16 rounding at the end."""
    h = x.float() if res is None else x.float() + res.float()
    ss = (h * h).sum(dim=1, keepdim=True, dtype=torch.float32)
    inv = torch.rsqrt(ss / h.shape[1] + torch.tensor(eps))
    return (h * inv * w.float()).bfloat16()


# ---------------------------------------------------------------------------
# rope

ROPE_CTX = 128
ROPE_T = (1, 3, 17)
ROPE_HEADS = ((4, 2), (7, 1), (3, 3))      # (Hq, Hk): T * Htot % 4 != 0 occurs


def rope_positions(T, ctx=ROPE_CTX, seed=0):
    """Seeded draw with ctx - 1 first and 0 second (T = 1: ctx - 1 alone):
    neither ascending nor equal to the row index."""
    g = torch.Generator().manual_seed(50 + seed + T)
    p = torch.randint(0, ctx, (T,), generator=g)
    p[0] = ctx - 1
    if T > 1:
        p[1] = 0
    return p.int()


def code_tables(ctx=ROPE_CTX, seed=0):
    """cos/sin [ctx, 64] fp32 holding a seeded code per (position, lane)
    from {(1,0), (0,1), (-1,0), (0,-1)}: every rotated element is +-x1 or
    +-x2 exactly, so a wrong position, lane or table stride shows as a bit
    difference.  Position 0 is the identity."""
    g = torch.Generator().manual_seed(60 + seed)
    code = torch.randint(0, 4, (ctx, D // 2), generator=g)
    code[0] = 0
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[code]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[code]
    return cos.contiguous(), sin.contiguous()


def rope_inputs(T, Hq, Hk, seed=0):
    s = 1000 * T + 10 * Hq + Hk + seed
    return (fo.rand_bf16(T, Hq, D, seed=s), fo.rand_bf16(T, Hk, D, seed=s + 1),
            fo.rand_bf16(T, Hk, D, seed=s + 2))


def fused_views(q, k, v=None):
    """q, k (and v) copied into one [T, (Hq + 2 Hk) * 128] buffer; returns
    (buf, q view, k view, v view).  Without v its columns are NaN."""
    T, Hq, _ = q.shape
    Hk = k.shape[1]
    buf = torch.full((T, (Hq + 2 * Hk) * D), float("nan"), dtype=q.dtype,
                     device=q.device)
    buf[:, :Hq * D] = q.reshape(T, -1)
    buf[:, Hq * D:(Hq + Hk) * D] = k.reshape(T, -1)
    if v is not None:
        buf[:, (Hq + Hk) * D:] = v.reshape(T, -1)
    return (buf, buf[:, :Hq * D].view(T, Hq, D),
            buf[:, Hq * D:(Hq + Hk) * D].view(T, Hk, D),
            buf[:, (Hq + Hk) * D:].view(T, Hk, D))


def emulate_rope(t, positions, cos, sin):
    """fp32 products and sum, one bf16 rounding."""
    c = cos[positions.long()].unsqueeze(1)
    s = sin[positions.long()].unsqueeze(1)
    lo, hi = t.float()[..., :64], t.float()[..., 64:]
    return torch.cat([lo * c - hi * s, hi * c + lo * s], dim=-1).bfloat16()


# ---------------------------------------------------------------------------
# adversarial append pool

APPEND_CAP = 48                 # positions per slot: 3 pages of 16
APPEND_SEQS = 3
APPEND_POS = (0, 15, 16, 17, 31, 32, APPEND_CAP - 1)


def _pattern(shape, seed):
    """Seeded finite bf16 bit patterns (random sign, exponent in
    [2^-27, 2^13), random mantissa)."""
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, shape, generator=g)
    exp = torch.randint(100, 140, shape, generator=g)
    man = torch.randint(0, 128, shape, generator=g)
    b = (sign << 15) | (exp << 7) | man
    return (b - (b >= 32768) * 65536).to(torch.int16).view(torch.bfloat16)


def append_pool(KVH, seed=0):
    """attn_oracle's adversarial pool (shuffled non-ascending page ids,
    slots a shuffled subset of 64, 3 layers with the tested one in the
    middle) for APPEND_SEQS slots of APPEND_CAP positions, with every
    element of both pools, in every layer, overwritten by a seeded finite
    bf16 pattern instead of zeros: each 128-row of either pool is distinct
    (the CPU file asserts it), so a write of zeros, a write to the right
    offset of the wrong page and a row copied from elsewhere all show."""
    z = torch.zeros(APPEND_CAP, KVH, D, dtype=torch.bfloat16)
    pool = ao.build_pool([(z, z)] * APPEND_SEQS, seed=300 + seed)
    c = pool.cache
    c.k_pool.copy_(_pattern(c.k_pool.shape, 2 * seed + 11))
    c.v_pool.copy_(_pattern(c.v_pool.shape, 2 * seed + 12))
    return pool


def append_batch(pool, kind, seed=0):
    """(slots [T], positions [T]) int32.  "mixed": every APPEND_POS of all
    three slots in one shuffled batch; "decode": T = S, one token per slot
    at different positions."""
    if kind == "decode":
        pairs = [(0, 17), (1, 0), (2, APPEND_CAP - 1)]
    else:
        pairs = [(s, p) for s in range(APPEND_SEQS) for p in APPEND_POS]
        g = torch.Generator().manual_seed(70 + seed)
        pairs = [pairs[i] for i in torch.randperm(len(pairs), generator=g)]
    slots = torch.tensor([pool.slots[s] for s, _ in pairs], dtype=torch.int32)
    pos = torch.tensor([p for _, p in pairs], dtype=torch.int32)
    return slots, pos


def pool_after(pool_tensor, page_table, slots, pos, rows):
    """The pool (CPU, [L, P, KVH, 16, 128]) after rows [T, KVH, 128] land
    at (slots, pos) of layer ao.LAYER; everything else keeps its pre-fill."""
    out = pool_tensor.clone()
    layer, pg, off = fo.paged_coords(page_table, slots, pos, ao.PAGE,
                                     ao.LAYER)
    out[layer, pg, :, off] = rows.to(out.dtype)
    return out


# ---------------------------------------------------------------------------
# swiglu

# the last case has 526 336 16-byte vectors, above the 2048 x 256 = 524 288
# threads of the launch: the grid-stride loop runs a second pass
SWIGLU_CASES = ((1, 8), (5, 1024), (3, 9472), (257, 16384))
SWIGLU_GATES = (100.0, -100.0, 88.0, -88.0, 0.0, -0.0)


def swiglu_inputs(T, F):
    """[T, 2F] = [gate | up] N(0,1) bf16; row 0 opens with the gates where
    exp(-g) overflows, saturates or vanishes."""
    gu = fo.rand_bf16(T, 2 * F, seed=F + T)
    gu[0, :len(SWIGLU_GATES)] = torch.tensor(SWIGLU_GATES).bfloat16()
    return gu


def emulate_swiglu(gu):
    F = gu.shape[1] // 2
    g, u = gu.float()[:, :F], gu.float()[:, F:]
    return (g * (1.0 / (1.0 + torch.exp(-g))) * u).bfloat16()


# ---------------------------------------------------------------------------
# row_sumsq

SUMSQ_H = (8, 2048, 2056, 3584, 8192)
SUMSQ_M = (1, 33)


# ---------------------------------------------------------------------------
# argmax: planted ties

LOW, HIGH = -5.0, 3.0
ARGMAX_V = 4104
# 768 // B slices: 385 and 769 give the single-block kernel, 384 two slices
# of 4096, everything else slices of 2048
ARGMAX_B = (1, 25, 32, 64, 384, 385, 769)
ARGMAX_SMALL_V = (7, 513, 2049)            # the slices collapse to one
ARGMAX_ODD_V = (4101, 32 * 2048 + 5)       # V % 8 != 0 behind full slices
ARGMAX_BIG_V = 128256
ARGMAX_BIG_B = (1, 32)


def tie_pairs(V):
    """(a, b), a < b < V, both holding the row maximum; a must win.  Same
    thread in two rounds of 2048, adjacent lanes, lanes 63 | 64 (waves 0 |
    1), 2047 | 2048, both ends, and around every multiple m of 2048: (m -
    1, m) straddles a slice or round edge, (m, m + 2047) spans one."""
    pairs = [(8, 8 + 2048), (7, 8), (511, 512), (2047, 2048), (0, V - 1)]
    for m in range(2048, V + 1, 2048):
        pairs += [(m - 1, m), (m, m + 2047)]
    out = []
    for a, b in pairs:
        if 0 <= a < b < V and (a, b) not in out:
            out.append((a, b))
    return out


def edge_indices(V):
    return sorted({i for p in tie_pairs(V) for i in p} | {0, V - 1})


def argmax_rows(V, ties_only=False):
    """([R, V] bf16 logits, [R] expected lowest-index argmax).  One row
    per tie pair (LOW everywhere, HIGH planted), then a single maximum at
    V - 1, an all -inf row and a row that is -inf except one finite entry
    three from the end (the last slice)."""
    pairs = tie_pairs(V)
    extra = 0 if ties_only else 3
    rows = torch.full((len(pairs) + extra, V), LOW)
    for r, (a, b) in enumerate(pairs):
        rows[r, a] = rows[r, b] = HIGH
    if not ties_only:
        n = len(pairs)
        rows[n, V - 1] = HIGH
        rows[n + 1] = float("-inf")
        rows[n + 2] = float("-inf")
        rows[n + 2, max(0, V - 3)] = -7.0
    expected = torch.from_numpy(np.argmax(rows.numpy(), axis=1))
    return rows.bfloat16(), expected


def batches(R, B):
    """Row indices of the launches that show every one of R rows at batch
    size B (the last launch wraps round)."""
    return [[(s + i) % R for i in range(B)] for s in range(0, R, B)]


# ---------------------------------------------------------------------------
# the sampler's counter noise, bit for bit
#
# key = seed * GOLD ^ ctr * CTRMUL ^ v (uint64, wrapping; the int64 seed
# reinterpreted, ctr through `unsigned`), the murmur3 fmix64 finaliser, and
# u = (float(key >> (64 - U_BITS)) + 0.5f) * 2^-U_BITS in float32.

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
CTRMUL = 0xD1B54A32D192ED03
FMIX1 = 0xFF51AFD7ED558CCD
FMIX2 = 0xC4CEB9FE1A85EC53
U_BITS = 23                      # the parent commit used 24 and reached u = 1


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.int64)).view(np.uint64)


def fmix64(k):
    """uint64 array -> uint64 array."""
    s = np.uint64(33)
    k = k ^ (k >> s)
    k = k * np.uint64(FMIX1)
    k = k ^ (k >> s)
    k = k * np.uint64(FMIX2)
    return k ^ (k >> s)


def hash_key(seed, ctr, v):
    """The finalised 64-bit key; seed (int64), ctr (int32) and v broadcast
    against each other."""
    sd = _u64(seed)
    ct = (np.atleast_1d(np.asarray(ctr, dtype=np.int64))
          & np.int64(0xFFFFFFFF)).astype(np.uint64)
    vv = np.atleast_1d(np.asarray(v, dtype=np.int64)).astype(np.uint64)
    return fmix64((sd * np.uint64(GOLD)) ^ (ct * np.uint64(CTRMUL)) ^ vv)


def u01_of_mantissa(m, nbits=U_BITS):
    """The kernel's uniform mapping of the key's top nbits, in float32."""
    m = np.asarray(m).astype(np.float32)
    return (m + np.float32(0.5)) * np.float32(2.0 ** -nbits)


def hash_u01(seed, ctr, v, nbits=U_BITS):
    return u01_of_mantissa(hash_key(seed, ctr, v) >> np.uint64(64 - nbits),
                           nbits)


def row_noise(seeds, ctrs, V, nbits=U_BITS):
    """[B, V] float32 u of a batch."""
    return hash_u01(np.asarray(seeds, dtype=np.int64)[:, None],
                    np.asarray(ctrs, dtype=np.int64)[:, None],
                    np.arange(V, dtype=np.int64)[None, :], nbits)


def gumbel_scores(logits, T, u):
    """fp64 l / T - log(-log(u)) per row; rows with T <= 0 are greedy and
    keep the plain logits.  logits [B, V] bf16 tensor, T [B], u [B, V]."""
    l = logits.double().numpy()
    T = np.asarray(T, dtype=np.float64).reshape(-1, 1)
    u = np.asarray(u, dtype=np.float64)
    samp = T > 0
    return np.where(samp, l / np.where(samp, T, 1.0) - np.log(-np.log(u)), l)


def emulate_gumbel_f32(logits, T, u):
    """The kernel's own order in float32: l * (1 / T) + g."""
    l = logits.float().numpy()
    T = np.asarray(T, dtype=np.float32).reshape(-1, 1)
    inv = np.float32(1.0) / np.where(T > 0, T, np.float32(1.0))
    g = -np.log(-np.log(np.asarray(u, dtype=np.float32)))
    return (l * inv + np.where(T > 0, g, np.float32(0.0))).astype(np.float32)


def _unxs(x):
    return x ^ (x >> 33)         # x ^= x >> 33 is its own inverse (66 > 64)


def solve_seed(ctr, v, top_bits, nbits=24, low=0x2545F4914F):
    """The int64 seed whose hash at (ctr, v) has `top_bits` as its top
    `nbits` bits: the finaliser run backwards (multiplicative inverses mod
    2^64), then the key composition solved for the seed."""
    key = ((top_bits << (64 - nbits)) | (low & ((1 << (64 - nbits)) - 1)))
    x = _unxs(key & M64)
    x = _unxs(x * pow(FMIX2, -1, 1 << 64) & M64)
    x = _unxs(x * pow(FMIX1, -1, 1 << 64) & M64)
    x ^= ((ctr & 0xFFFFFFFF) * CTRMUL & M64) ^ v
    s = x * pow(GOLD, -1, 1 << 64) & M64
    return s - (1 << 64) if s >> 63 else s


# the parent's mapping gives u == 1 here: all 24 top bits set at ctr 0, v 5
POISON_SEED = -7087549625518640403
POISON_CTR, POISON_V = 0, 5
POISON2_CTR = 4095               # second poison: aimed at v = V - 1
REGRESSION_V = (64, 4104)


def regression_case(V, which):
    """logits [3, V] (0 at token 0, -30 elsewhere), seeds, ctrs; the middle
    row's hash has all 24 top bits set at one token.  A finite Gumbel
    noise lies in [-2.82, 16.64], so no token can make up 30: every row
    must return 0."""
    logits = torch.full((3, V), -30.0)
    logits[:, 0] = 0.0
    if which == 0:
        seed, ctr = POISON_SEED, POISON_CTR
    else:
        seed, ctr = solve_seed(POISON2_CTR, V - 1, (1 << 24) - 1), POISON2_CTR
    seeds = torch.tensor([1, seed, -2], dtype=torch.int64)
    ctrs = torch.tensor([ctr, ctr, ctr], dtype=torch.int32)
    return logits.bfloat16(), seeds, ctrs


# ---- counter-mode cases ----------------------------------------------------

# 50257 gives an odd slice length, B = 400 a single slice (768 // B = 1)
GUMBEL_CASES = ((1, 64), (7, 50257), (32, 4104), (4, 128256), (400, 520))
SEED_POOL = (0, 1, -1, 2 ** 63 - 1, -2 ** 63, -7046029254386353131,
             0x123456789ABC, 99)
CTR_POOL = (0, 1, 4095, 2 ** 31 - 1)
TEMP_POOL = (0.7, 1.0, 1.3)
GREEDY_HIGH = 12.0

# Decision margin.  The float32 emulation of l * (1/T) + g differs from the
# fp64 scores by at most 9.57e-7 over all GUMBEL_CASES (measured by
# tests/test_elem_oracle_cpu.py, which holds the constant to it; scores
# reach +-30, where half a float32 ulp is 9.5e-7); 16 x that covers __logf,
# whose error on gfx950 nobody has measured here.  Rows whose fp64
# best-to-runner-up gap is below GUMBEL_GAMMA = 1.6e-5 may pick either of
# the two; the smallest gap of any case is 1.8e-5.
GUMBEL_F32_ERR = 1.0e-6
GUMBEL_GAMMA = 16 * GUMBEL_F32_ERR


@functools.lru_cache(maxsize=None)
def gumbel_case(B, V):
    """logits [B, V] bf16 (N(0, 1.5)), temps [B] fp32, seeds [B] int64,
    ctrs [B] int32.  With B >= 4 rows 0..3 share logits and temperature:
    row 1 repeats row 0's (seed, ctr), row 2 differs in the seed only,
    row 3 in ctr only.  With B >= 7 rows 5 and 6 of every 7 are greedy
    (T = 0 and T = -1) with two planted equal maxima."""
    o = GUMBEL_CASES.index((B, V))
    logits = fo.rand_bf16(B, V, scale=1.5, seed=900 + o)
    si = [(r + 2 * o + 2) % len(SEED_POOL) for r in range(B)]
    ci = [(r // 2 + o + 3) % len(CTR_POOL) for r in range(B)]
    temps = [TEMP_POOL[r % 3] for r in range(B)]
    if B >= 4:
        logits[1:4] = logits[0]
        temps[1:4] = [temps[0]] * 3
        si[1], ci[1] = si[0], ci[0]
        si[2], ci[2] = (si[0] + 1) % len(SEED_POOL), ci[0]
        si[3], ci[3] = si[0], (ci[0] + 1) % len(CTR_POOL)
    if B >= 7:
        ties = ((0, V - 1), (7, 8), (V // 2 - 1, V // 2), (V - 2, V - 1))
        for r in range(B):
            if r % 7 >= 5:
                temps[r] = 0.0 if r % 7 == 5 else -1.0
                a, b = ties[(r // 7) % len(ties)]
                logits[r, a] = logits[r, b] = GREEDY_HIGH
    return (logits, torch.tensor(temps, dtype=torch.float32),
            torch.tensor([SEED_POOL[i] for i in si], dtype=torch.int64),
            torch.tensor([CTR_POOL[i] for i in ci], dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def gumbel_expected(B, V):
    """(best [B], runner [B], gap [B] fp64, f32_err): the fp64 argmax of
    the scores under the emulated noise, the runner-up and their gap (inf
    on greedy rows, whose best is the lowest-index maximum), and the
    largest |float32 emulation - fp64 score| over the sampled rows."""
    logits, temps, seeds, ctrs = gumbel_case(B, V)
    u = row_noise(seeds.numpy(), ctrs.numpy(), V)
    sc = gumbel_scores(logits, temps.numpy(), u)
    best = np.argmax(sc, axis=1)
    rest = sc.copy()
    rest[np.arange(B), best] = -np.inf
    runner = np.argmax(rest, axis=1)
    gap = sc[np.arange(B), best] - sc[np.arange(B), runner]
    samp = temps.numpy() > 0
    gap = np.where(samp, gap, np.inf)
    err = np.abs(emulate_gumbel_f32(logits, temps.numpy(), u).astype(
        np.float64) - sc)[samp]
    return best, runner, gap, float(err.max()) if err.size else 0.0
