"""fp64 oracle, adversarial paged pools, fp32 kernel emulations, budgets
and case lists for the paged attention kernels (tests/test_attn_oracle_cpu.py
proves them on the CPU, tests/test_attention_gpu.py applies them to
k_decode_attn / k_decode_combine / k_prefill_attn / k_paged_attn<16>).

Everything here is plain torch on the CPU.  The oracle takes the SAME bf16
q/k/v the kernels see, upcast to double, so the only legitimate difference
is fp32 arithmetic order, the bf16 rounding of the output and, for the
MFMA prefill, the bf16 rounding of P.

Three tiers of inputs:
  A1 probes    keys are 32 x (+-1 codes), the query is one key's code: the
               softmax is exactly one-hot in fp32, so the output must be
               that key's V row bit for bit (positive probe), or, when the
               probed key is invisible, the oracle over the visible keys.
  A2 counting  K = 0 and one-hot V rows: every visible key weighs exactly
               1, the output is (keys with j % 128 == d) / n_visible.
  B  real      N(0,1) k/v, q at scale 1 and 3, held to the budgets below.
"""
import functools
import math

import torch

import fused_oracle as fo
from ollamamq_amd.engine.kvcache import PagedKVCache
from ollamamq_amd.ops.interface import AttnMeta

D = 128
PAGE = 16
LAYERS = 3            # the tested layer is neither the first nor the last
LAYER = 1
SCALE = 1.0 / math.sqrt(D)
NEG = -3.0e38         # the kernels' "masked" score


# ---------------------------------------------------------------------------
# adversarial paged pool


class Pool:
    """A PagedKVCache whose page table and pools were written directly.

    K[i], V[i] ([n_i, KVH, 128] bf16) are the rows sequence i owns, at
    positions 0..n_i-1 of slot slots[i].  Everything else in k_pool and
    v_pool, in every layer, is NaN, and every page-table entry that is not
    an owned page points at an all-NaN spare page: a kernel that strays
    returns NaN instead of agreeing by accident (or faulting)."""

    def __init__(self, cache, slots, K, V):
        self.cache, self.slots, self.K, self.V = cache, slots, K, V
        self.KVH = K[0].shape[1]

    def to(self, device):
        c = self.cache
        g = PagedKVCache(LAYERS, self.KVH, D, page_size=PAGE,
                         n_pages=c.n_pages, max_slots=c.max_slots,
                         max_ctx=c.max_ctx, device=device,
                         dtype=torch.bfloat16)
        g.k_pool.copy_(c.k_pool)
        g.v_pool.copy_(c.v_pool)
        g.page_table.copy_(c.page_table)
        return Pool(g, self.slots, self.K, self.V)

    def meta(self, seqs, seq_lens, q_lens=None, window=0, max_kv=None,
             mode=None, n_decode=0):
        """AttnMeta for batch rows reading sequences `seqs` (indices into
        K/V; several rows may share one) at KV lengths `seq_lens`."""
        q_lens = list(q_lens) if q_lens is not None else [1] * len(seqs)
        cu = [0]
        for n in q_lens:
            cu.append(cu[-1] + n)
        dev = self.cache.page_table.device
        if mode is None:
            mode = "decode" if max(q_lens) == 1 else "prefill"
        return AttnMeta(
            mode=mode,
            slot_ids=torch.tensor([self.slots[i] for i in seqs],
                                  dtype=torch.int32, device=dev),
            seq_lens=torch.tensor(list(seq_lens), dtype=torch.int32,
                                  device=dev),
            cu_q=torch.tensor(cu, dtype=torch.int32, device=dev),
            logits_idx=None, max_q=max(q_lens),
            max_kv=max_kv or max(seq_lens), n_decode=n_decode,
            window=window)


def build_pool(kvs, seed=0, max_ctx=None, max_slots=64):
    """kvs: [(K_i, V_i)] with K_i, V_i [n_i, KVH, 128] bf16 -> Pool.

    Slots are a shuffled subset of max_slots (never 0, 1, 2, ...), page
    ids a seeded permutation that is not ascending within any slot.
    max_slots stays above every batch size the tests launch, so even a
    page-table row indexed by batch row lands on the spare NaN page."""
    g = torch.Generator().manual_seed(1000 + seed)
    n = len(kvs)
    KVH = kvs[0][0].shape[1]
    need = [(K.shape[0] + PAGE - 1) // PAGE for K, _ in kvs]
    max_ctx = max_ctx or PAGE * max(need)
    assert max_ctx >= PAGE * max(need) and n < max_slots
    n_pages = sum(need) + 5
    cache = PagedKVCache(LAYERS, KVH, D, page_size=PAGE, n_pages=n_pages,
                         max_slots=max_slots, max_ctx=max_ctx, device="cpu",
                         dtype=torch.bfloat16)
    while True:
        slots = torch.randperm(max_slots, generator=g)[:n].tolist()
        if slots != list(range(n)):
            break
    perm = torch.randperm(n_pages, generator=g).tolist()
    spare = perm[-1]
    cache.page_table.fill_(spare)
    cache.k_pool.fill_(float("nan"))
    cache.v_pool.fill_(float("nan"))
    at = 0
    for i, (K, V) in enumerate(kvs):
        pages = perm[at:at + need[i]]
        at += need[i]
        if len(pages) >= 2 and pages == sorted(pages):
            pages[0], pages[-1] = pages[-1], pages[0]
        assert len(pages) < 2 or pages != sorted(pages)
        pt = torch.tensor(pages, dtype=torch.int32)
        cache.page_table[slots[i], :len(pages)] = pt
        pos = torch.arange(K.shape[0])
        pg, off = pt[pos // PAGE].long(), pos % PAGE
        cache.k_pool[LAYER, pg, :, off] = K
        cache.v_pool[LAYER, pg, :, off] = V
    assert spare not in set(perm[:at])
    return Pool(cache, slots, [k for k, _ in kvs], [v for _, v in kvs])


# ---------------------------------------------------------------------------
# fp64 oracle


def visible(q_pos, kv_len, window, n_keys):
    """[Q, n_keys] bool: the query at position p sees keys
    [max(0, p - window + 1), p] below kv_len (window 0 = full causal)."""
    kp = torch.arange(n_keys).unsqueeze(0)
    qp = torch.as_tensor(q_pos).reshape(-1, 1)
    vis = (kp <= qp) & (kp < kv_len)
    if window > 0:
        vis &= kp >= qp - window + 1
    return vis


def attention_oracle(q, K, V, q_pos, kv_len, window=0, vis=None):
    """One sequence.  q [Q, Hq, 128], K/V [n, KVH, 128] (n >= kv_len; rows
    past kv_len are only reachable through an explicit `vis`), q_pos the
    Q absolute query positions.  `vis` ([Q, n] or [Hq, Q, n] bool)
    replaces the rule above; the sensitivity tests edit it.
    Returns (out, absP) fp64 [Q, Hq, 128]: softmax(S) @ V and
    softmax(S) @ |V|."""
    Hq, KVH, n = q.shape[1], K.shape[1], K.shape[0]
    G = Hq // KVH
    if vis is None:
        vis = visible(q_pos, kv_len, window, n)
    Kd = K.double().repeat_interleave(G, dim=1)
    Vd = V.double().repeat_interleave(G, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.double(), Kd) * SCALE
    s = s.masked_fill(~vis.expand(Hq, -1, -1), float("-inf"))
    p = torch.softmax(s, dim=-1)
    return (torch.einsum("hqk,khd->qhd", p, Vd),
            torch.einsum("hqk,khd->qhd", p, Vd.abs()))


def oracle_batch(pool, q, seqs, seq_lens, q_lens=None, window=0):
    """The oracle over a flat varlen batch laid out like AttnMeta."""
    q_lens = list(q_lens) if q_lens is not None else [1] * len(seqs)
    outs, absps, at = [], [], 0
    for i, n, ql in zip(seqs, seq_lens, q_lens):
        o, a = attention_oracle(q[at:at + ql], pool.K[i], pool.V[i],
                                list(range(n - ql, n)), n, window)
        outs.append(o)
        absps.append(a)
        at += ql
    return torch.cat(outs), torch.cat(absps)


def oracle_from_cache(q, cache, layer, slots, seq_lens, q_lens, window=0):
    """The oracle over a batch whose K/V sit in an ordinary CPU cache."""
    from ollamamq_amd.ops.reference import _gather_kv
    outs, absps, at = [], [], 0
    for slot, n, ql in zip(slots, seq_lens, q_lens):
        K, V = _gather_kv(cache, layer, slot, n)
        o, a = attention_oracle(q[at:at + ql].cpu(), K, V,
                                list(range(n - ql, n)), n, window)
        outs.append(o)
        absps.append(a)
        at += ql
    return torch.cat(outs), torch.cat(absps)


# ---------------------------------------------------------------------------
# budgets
#
# Decode and the VALU kernel keep p in fp32: |err| <= 2^-7 |t| + 2^-8 rms(t)
# (fused_oracle.assert_bf16_close, unchanged).  The MFMA prefill rounds P
# to bf16 before the PV MFMA while l sums the unrounded p, so each p carries
# a relative error <= 2^-9 and an output element moves by at most
# 2^-9 * sum_j p_j |v_j| / l = 2^-9 * absP on top of that.  The rms is taken
# per sequence (never across sequences of different length, whose output
# magnitudes differ by 10x), which only tightens the budget.


def ratio(got, truth, absP=None, per_vector=False):
    """Worst |got - truth| / budget; per_vector takes the rms over the
    last dim only (one 128-vector at a time).  inf on a non-finite
    output."""
    g, t = got.detach().double().cpu(), truth.detach().double().cpu()
    assert g.shape == t.shape, f"shape {g.shape} vs {t.shape}"
    if not torch.isfinite(g).all():
        return float("inf")
    rms = t.pow(2).mean(dim=-1, keepdim=True).sqrt() if per_vector \
        else t.pow(2).mean().sqrt()
    budget = t.abs() * 2.0 ** -7 + rms * 2.0 ** -8
    if absP is not None:
        budget = budget + absP.double() * 2.0 ** -9
    err = (g - t).abs()
    bad = (budget == 0) & (err > 0)
    if bad.any():
        return float("inf")
    return float((err / budget.clamp_min(1e-300)).max())


def assert_close(got, truth, q_lens, absP=None, what=""):
    """Per sequence: decode/VALU budget (fo.assert_bf16_close) or, with
    absP, the prefill budget.  Returns the worst normalised error."""
    worst, at = 0.0, 0
    g = got.detach().cpu()
    assert g.shape == truth.shape, f"{what}: {g.shape} vs {truth.shape}"
    for i, ql in enumerate(q_lens):
        sl = slice(at, at + ql)
        tag = f"{what} seq {i}"
        if absP is None:
            w = fo.assert_bf16_close(g[sl], truth[sl], tag)
        else:
            assert torch.isfinite(g[sl]).all(), f"{tag}: non-finite output"
            w = ratio(g[sl], truth[sl], absP[sl])
            assert w <= 1.0, f"{tag}: worst normalised error {w:.3f}"
        worst = max(worst, w)
        at += ql
    assert at == g.shape[0]
    return worst


# ---------------------------------------------------------------------------
# fp32 emulations of the kernels' arithmetic (chunked online softmax,
# floor-interpolated segment bounds, (o, m, l) combine).  They exist to
# show that the budgets hold for a correct fp32 implementation and are
# not fitted to the kernels.


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def decode_segments(kv_len, window, CH, split):
    """(lo_tok, [(c0, c1)]) exactly as k_decode_attn derives them."""
    n_chunks = (kv_len + CH - 1) // CH
    lo = kv_len - window if (window > 0 and kv_len > window) else 0
    cb = lo // CH
    n_act = n_chunks - cb
    return lo, [(cb + n_act * s // split, cb + n_act * (s + 1) // split)
                for s in range(split)]


def emulate_decode(q, K, V, kv_len, window, CH, split):
    """q [Hq, 128] bf16 -> [Hq, 128] bf16."""
    Hq, G = q.shape[0], q.shape[0] // K.shape[1]
    qf = q.float()
    Kf = K.float().repeat_interleave(G, dim=1)
    Vf = V.float().repeat_interleave(G, dim=1)
    sc = _f32(SCALE)
    lo, segs = decode_segments(kv_len, window, CH, split)
    parts = []
    for c0, c1 in segs:
        m = torch.full((Hq,), NEG)
        l = torch.zeros(Hq)
        o = torch.zeros(Hq, D)
        for ch in range(c0, c1):
            idx = torch.arange(max(ch * CH, lo), min(ch * CH + CH, kv_len))
            s = torch.einsum("khd,hd->hk", Kf[idx], qf) * sc
            mn = torch.maximum(m, s.max(dim=1).values)
            corr = torch.exp(m - mn)
            p = torch.exp(s - mn.unsqueeze(1))
            l = l * corr + p.sum(dim=1)
            o = o * corr.unsqueeze(1) + torch.einsum("hk,khd->hd", p, Vf[idx])
            m = mn
        parts.append((o, m, l))
    if split > 1:
        mm = torch.stack([m for _, m, _ in parts]).max(dim=0).values
        l = torch.zeros(Hq)
        o = torch.zeros(Hq, D)
        for oi, mi, li in parts:
            w = torch.where(mi <= NEG, torch.zeros(Hq), torch.exp(mi - mm))
            l = l + w * li
            o = o + w.unsqueeze(1) * oi
    linv = torch.where(l > 0, 1.0 / l, torch.zeros(Hq))
    return (o * linv.unsqueeze(1)).bfloat16()


def emulate_prefill(q, K, V, pos0, window, CH=64, round_p=True):
    """q [Q, Hq, 128] bf16 at positions pos0.. -> [Q, Hq, 128] bf16, in
    32-row tiles like k_prefill_attn; round_p rounds P to bf16 before the
    PV product while l keeps the unrounded sum."""
    Q, Hq = q.shape[0], q.shape[1]
    G = Hq // K.shape[1]
    Kf = K.float().repeat_interleave(G, dim=1)
    Vf = V.float().repeat_interleave(G, dim=1)
    sc = _f32(SCALE)
    out = torch.empty(Q, Hq, D, dtype=torch.bfloat16)
    for t0 in range(0, Q, 32):
        rows = min(32, Q - t0)
        p0 = pos0 + t0
        kv_len = p0 + rows
        qf = q[t0:t0 + rows].float()
        qpos = torch.arange(p0, p0 + rows).unsqueeze(1)
        n_chunks = (kv_len + CH - 1) // CH
        ch_lo = (p0 - window + 1) // CH if (window > 0 and p0 >= window) \
            else 0
        m = torch.full((Hq, rows), NEG)
        l = torch.zeros(Hq, rows)
        o = torch.zeros(Hq, rows, D)
        for ch in range(ch_lo, n_chunks):
            idx = torch.arange(ch * CH, min(ch * CH + CH, kv_len))
            ok = idx.unsqueeze(0) <= qpos
            if window > 0:
                ok &= idx.unsqueeze(0) > qpos - window
            s = torch.einsum("qhd,khd->hqk", qf, Kf[idx]) * sc
            s = torch.where(ok, s, _f32(NEG))
            mn = torch.maximum(m, s.max(dim=-1).values)
            corr = torch.exp(m - mn)
            p = torch.where(ok, torch.exp(s - mn.unsqueeze(-1)),
                            torch.zeros(()))
            l = l * corr + p.sum(dim=-1)
            pv = p.bfloat16().float() if round_p else p
            o = o * corr.unsqueeze(-1) + torch.einsum("hqk,khd->hqd", pv,
                                                      Vf[idx])
            m = mn
        linv = torch.where(l > 0, 1.0 / l, torch.zeros(()))
        out[t0:t0 + rows] = (o * linv.unsqueeze(-1)).permute(1, 0, 2) \
            .bfloat16()
    return out


# ---------------------------------------------------------------------------
# shared case lists

# (G, KVH): every dispatched group at KVH = 2, plus KVH = 1 and KVH = 3
GROUPS = [(G, 2) for G in range(1, 9)] + [(8, 1), (3, 3)]

DECODE_LENS = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
DECODE_CHUNKS = (32, 64)
DECODE_SPLITS = (None, 1, 2, 3, 5)          # None = the wrapper's own choice
# hipGraph capture geometry: max_kv is the pool's max_ctx -> split 32 with
# n_act < split and mostly empty segments
CAPTURE_LENS = (1, 5, 70)
CAPTURE_MAX_KV = 4096
# (window, kv_lens): lo_tok = kv_len - W lands on 0, 1, a chunk edge (64)
# and one past it (65); W = 1 leaves exactly the last key
DECODE_WINDOWS = [(100, (40, 100, 101, 164, 165, 300)),
                  (64, (1, 63, 64, 65, 128, 129, 200)),
                  (1, (1, 16, 17, 65, 200))]
WINDOW_SPLITS = (1, 3)
S33_LENS = tuple((i * 37) % 130 + 1 for i in range(33))
Q_SCALES = (1.0, 3.0)

# (q_len, kv_len); the last three continue an earlier chunk: (33, 97) has
# pos0 = 64 so chunk 0 is interior, (1, 200) is a single-row tile
PREFILL_CASES = ((1, 1), (31, 31), (32, 32), (33, 33), (64, 64), (65, 65),
                 (130, 130), (23, 63), (33, 97), (1, 200))
# window prompts: 200 rows give tiles with ch_lo = 1 (odd: the first staged
# buffer is buffer 1) for every W below, and interior chunks inside the
# window at W = 96
PREFILL_WINDOWS = (1, 32, 64, 70, 96)
PREFILL_WINDOW_CASES = ((200, 200), (33, 97), (37, 37), (1, 200))

# three prefill chunks (one continued) after three decode rows
MIXED_DECODE_LENS = (17, 65, 200)
MIXED_PREFILL = ((40, 40), (33, 97))
MIXED_WINDOWS = (0, 70)


def wrapper_split(S, KVH, max_kv, forced=None):
    """The split attention_decode derives (forced = OLLAMAMQ_DECODE_SPLIT)."""
    want = forced or max(1, 1024 // max(1, S * KVH))
    return int(min(want, max(1, (max_kv + 63) // 64), 32))


def decode_groups(G):
    """(tag, kv_lens, window, splits, max_kv) of the tier-B decode runs of
    one GQA group; split None leaves the choice to the wrapper.  max_kv is
    an upper bound the wrapper only sizes the split from: forced splits
    get 512 so that it does not clamp them."""
    groups = [("plain", DECODE_LENS, 0, (None,), max(DECODE_LENS)),
              ("forced", DECODE_LENS, 0, DECODE_SPLITS[1:], 512),
              ("capture", CAPTURE_LENS, 0, (None,), CAPTURE_MAX_KV)]
    for W, lens in DECODE_WINDOWS:
        groups.append((f"W{W}", lens, W, WINDOW_SPLITS, 512))
    if G == 4:
        groups.append(("S33", S33_LENS, 0, (1, 3), 512))
    return groups


def case_seed(G, KVH, tag):
    return G * 100 + KVH * 10 + tag


def real_kv(lens, KVH, seed):
    return [(fo.rand_bf16(n, KVH, D, seed=seed * 1000 + 2 * i),
             fo.rand_bf16(n, KVH, D, seed=seed * 1000 + 2 * i + 1))
            for i, n in enumerate(lens)]


def real_q(T, Hq, scale, seed):
    return fo.rand_bf16(T, Hq, D, scale=scale, seed=seed * 1000 + 999)


def decode_inputs(G, KVH, gi, lens, scale):
    """(kvs, q [S, Hq, 128]) of decode group number gi."""
    seed = case_seed(G, KVH, gi)
    return (real_kv(lens, KVH, seed),
            real_q(len(lens), G * KVH, scale, seed + int(scale)))


def prefill_runs():
    return [(0, PREFILL_CASES)] + \
        [(W, PREFILL_WINDOW_CASES) for W in PREFILL_WINDOWS]


def prefill_inputs(G, KVH, wi, cases, scale):
    """(kvs, q [T, Hq, 128]) of prefill run number wi."""
    seed = case_seed(G, KVH, 20 + wi)
    return (real_kv([n for _, n in cases], KVH, seed),
            real_q(sum(ql for ql, _ in cases), G * KVH, scale,
                   seed + int(scale)))


def strided(q, KVH, fill=float("nan")):
    """The same q as a view of a fused [T, (Hq + 2 KVH) * 128] qkv buffer
    whose k/v columns are NaN."""
    T, Hq, _ = q.shape
    buf = torch.full((T, (Hq + 2 * KVH) * D), fill, dtype=q.dtype,
                     device=q.device)
    buf[:, :Hq * D] = q.reshape(T, Hq * D)
    return buf[:, :Hq * D].view(T, Hq, D)


# ---- tier A1: probes -------------------------------------------------------

N_CODES = 640
PROBE_CAP = 320            # positions owned per probe sequence (20 pages)
PROBE_SEQS = 3
PROBE_DECODE_WINDOWS = (0, 100, 64)
PROBE_PREFILL_WINDOWS = (0, 32, 70)
MIN_GAP = 110.0            # exp(-110) < fp32's smallest denormal (e^-103.3)


@functools.lru_cache(maxsize=1)
def probe_codes():
    g = torch.Generator().manual_seed(1)
    h = (torch.randint(0, 2, (N_CODES, D), generator=g) * 2 - 1).float()
    gram = h @ h.t()
    gram.fill_diagonal_(0)
    maxdot = float(gram.abs().max())
    gap = (32 * D - 32 * maxdot) * SCALE
    assert gap >= MIN_GAP, (maxdot, gap)
    return h


def _code_of(seq, kvh, pos):
    return (pos + 211 * seq + 77 * kvh) % N_CODES


def probe_kv(KVH, seed=7):
    """PROBE_SEQS sequences of PROBE_CAP keys 32 * code; within one
    (sequence, kv head) every key has its own code, and V rows are
    distinct.  Rows past a test's kv_len are finite decoys."""
    h = probe_codes()
    pos = torch.arange(PROBE_CAP)
    kvs = []
    for s in range(PROBE_SEQS):
        K = torch.stack([32 * h[_code_of(s, k, pos)] for k in range(KVH)],
                        dim=1).bfloat16()
        V = fo.rand_bf16(PROBE_CAP, KVH, D, seed=seed * 100 + s)
        kvs.append((K, V))
    allv = torch.cat([v.reshape(-1, D) for _, v in kvs]).float()
    assert torch.unique(allv, dim=0).shape[0] == allv.shape[0]
    return kvs


def probe_q(seq, kvh, target):
    return probe_codes()[_code_of(seq, kvh, target)].bfloat16()


def decode_probe_plan(Hq, KVH, window):
    """Batch rows for the decode probes: (seqs, kv_lens, targets [S, Hq],
    positive [S, Hq] bool).  Positive targets: 0, 15, 16, 31, 32, 63, 64,
    65, kv_len - 1, lo_tok and every segment's first and last key under
    splits 2, 3, 5 at either chunk length; negative ones (the first
    invisible keys): kv_len and lo_tok - 1.  Each head of a row carries
    its own target; rows cycle through the probe sequences."""
    if window == 0:
        lens = (1, 16, 17, 64, 65, 66, 129, 200, 300)
    elif window == 100:
        lens = (40, 100, 101, 164, 165, 300)
    else:
        lens = (1, window, window + 1, 2 * window, 2 * window + 1, 200)
    seqs, kv_lens, targets, positive = [], [], [], []
    for n in lens:
        lo = n - window if (window > 0 and n > window) else 0
        pos = {0, 15, 16, 31, 32, 63, 64, 65, n - 1, lo}
        for CH in DECODE_CHUNKS:
            for split in (2, 3, 5):
                for c0, c1 in decode_segments(n, window, CH, split)[1]:
                    if c0 < c1:
                        pos.add(max(c0 * CH, lo))
                        pos.add(min(c1 * CH, n) - 1)
        pos = sorted(t for t in pos if lo <= t < n)
        neg = [t for t in (n, lo - 1) if 0 <= t < PROBE_CAP]
        items = [(t, True) for t in pos] + [(t, False) for t in neg]
        while len(items) % Hq:
            items.append(items[len(items) % len(pos)])
        for r in range(0, len(items), Hq):
            seqs.append(len(seqs) % PROBE_SEQS)
            kv_lens.append(n)
            targets.append([t for t, _ in items[r:r + Hq]])
            positive.append([p for _, p in items[r:r + Hq]])
    assert len(seqs) < 64
    return seqs, kv_lens, targets, positive


def prefill_probe_plan(Hq, cases, window):
    """Per query row and head one target: the diagonal p, the window edge
    p - W + 1, 0, 63, 64 (positive where visible) and the first invisible
    keys p + 1 and p - W (negative).  Returns (seqs, kv_lens, q_lens,
    targets [T, Hq], positive [T, Hq])."""
    seqs, kv_lens, q_lens, targets, positive = [], [], [], [], []
    for i, (ql, n) in enumerate(cases):
        seqs.append(i % PROBE_SEQS)
        kv_lens.append(n)
        q_lens.append(ql)
        for r in range(ql):
            p = n - ql + r
            lo = max(0, p - window + 1) if window > 0 else 0
            cand = [(p, True), (lo, True)]
            cand += [(t, True) for t in (0, 63, 64) if lo <= t <= p]
            if p + 1 < PROBE_CAP:
                cand.append((p + 1, False))
            if window > 0 and p - window >= 0:
                cand.append((p - window, False))
            row = [cand[(3 * r + h) % len(cand)] for h in range(Hq)]
            targets.append([t for t, _ in row])
            positive.append([s for _, s in row])
    return seqs, kv_lens, q_lens, targets, positive


def probe_queries(seqs, q_lens, targets, Hq, KVH):
    """[T, Hq, 128] bf16 queries for a plan."""
    G = Hq // KVH
    h = probe_codes()
    tg = torch.tensor(targets)
    seq_of_row = torch.tensor(
        [s for s, ql in zip(seqs, q_lens) for _ in range(ql)]).unsqueeze(1)
    kvh = (torch.arange(Hq) // G).unsqueeze(0)
    return h[_code_of(seq_of_row, kvh, tg)].bfloat16()


def probe_expected(pool, seqs, q_lens, targets, Hq):
    """[T, Hq, 128] bf16: V[target] of each (row, head)."""
    G = Hq // pool.KVH
    rows, at = [], 0
    for s, ql in zip(seqs, q_lens):
        tg = torch.tensor(targets[at:at + ql])
        kvh = (torch.arange(Hq) // G).expand_as(tg)
        rows.append(pool.V[s][tg, kvh])
        at += ql
    return torch.cat(rows)


# ---- tier A2: counting -----------------------------------------------------

COUNT_CAP = 528
COUNT_SEQS = 2
COUNT_DECODE_LENS = DECODE_LENS + (300, 516)


def counting_kv(KVH):
    """K = 0; V[j, h, d] = 1 where d == (j + 5 h + 3 seq) % 128."""
    kvs = []
    j = torch.arange(COUNT_CAP).unsqueeze(1)
    for s in range(COUNT_SEQS):
        hot = (j + 5 * torch.arange(KVH).unsqueeze(0) + 3 * s) % D
        V = torch.zeros(COUNT_CAP, KVH, D).scatter_(
            2, hot.unsqueeze(-1), 1.0).bfloat16()
        kvs.append((torch.zeros(COUNT_CAP, KVH, D).bfloat16(), V))
    return kvs


def assert_counting(got, truth, what=""):
    """Counting outputs: the decode budget per 128-vector (P = 1 is exact
    in bf16, so the prefill needs no P-rounding term) and exact zeros
    where no visible key feeds the element."""
    g = got.detach().cpu()
    assert torch.isfinite(g).all(), f"{what}: non-finite output"
    zero = truth == 0
    assert bool((g[zero] == 0).all()), f"{what}: nonzero where count is 0"
    w = ratio(g, truth, per_vector=True)
    assert w <= 1.0, f"{what}: worst normalised error {w:.3f}"
    return w
