"""fp64 model oracle, teacher-forced reference run, measured budgets,
trajectory check and pool helpers for the code that WIRES the kernels
together: LlamaModel.forward / _forward_decode_fused and the engine's decode
step (tests/test_model_oracle_cpu.py proves the yardstick on the CPU,
tests/test_model_forward_gpu.py and tests/test_engine_oracle_gpu.py apply
it on the GPU).

Method.  Tokens diverge once a near-tie flips, so free-running paths can
only be compared leniently.  Teacher forcing removes that: the oracle runs
on the tokens the GPU actually consumed and produced, so every step is
checked against truth at identical inputs.

  oracle     dense float64 Llama block over whole sequences, reading the
             model's own (bf16) tensors upcast to double: nothing paged,
             chunked or rounded.
  reference  the project's CPU path (bf16 model, ops/reference.py: fp32
             arithmetic, bf16 wherever an op returns), one prefill per
             sequence.  No HIP code.  Its error against the oracle is what
             a correct bf16-staged implementation costs.
  budget     per case and observable class (logits; K and V per layer):
             2 x the reference's worst row error at that case's tokens.
             The GPU path and the reference are two draws of the same
             process (as many bf16 roundings or fewer, another fp32
             summation order, bf16 P in the MFMA prefill), so their errors
             are alike in size but not equal; a wiring fault moves a row
             by O(rms), ~20 x the budget.
  row        one logits row, or the KVH x 128 K (V) values of one
             (layer, token).  rel = |got - truth|_2 / |truth|_2,
             mx = max|got - truth| / rms(truth).

Nothing here imports the GPU at module level.
"""
import functools
import math

import numpy as np
import torch

import attn_oracle as ao
import elem_oracle as eo
import fused_oracle as fo
from ollamamq_amd.engine.kvcache import PagedKVCache
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.models.llama import LlamaConfig
from ollamamq_amd.ops.interface import AttnMeta
from ollamamq_amd.ops.reference import _gather_kv

SEED = 1234
PAGE = 16
MAX_CTX = 256           # pool context of the forward-level rigs

# Two configs built here, not presets.  MHA mini: G = 1 takes the chunk-32
# decode attention.  Qwen-shaped mini: G = 7, 11 k-blocks (uneven wave
# ranges), 22 rstd tiles, down K = 19 blocks, a middle layer, qkv bias.
MINIS = {
    "mha-mini": LlamaConfig(
        name="mha-mini", n_layers=2, hidden=256, n_heads=2, n_kv_heads=2,
        head_dim=128, ffn=512, vocab=256, max_ctx=512, rope_theta=10000.0),
    "qwen-mini": LlamaConfig(
        name="qwen-mini", n_layers=3, hidden=704, n_heads=7, n_kv_heads=1,
        head_dim=128, ffn=1216, vocab=1056, max_ctx=512, rope_theta=10000.0,
        qkv_bias=True),
}
CONFIGS = ("tiny", "tiny-qwen", "tiny-swa", "mha-mini", "qwen-mini")


def config(name):
    return MINIS[name] if name in MINIS else PRESETS[name]


@functools.lru_cache(maxsize=None)
def cpu_model(name, dtype=torch.bfloat16, seed=SEED):
    """The project's CPU model: same seed, so the same bf16 weights as the
    GPU model (both round one CPU-generated fp32 draw)."""
    return LlamaModel(config(name), device="cpu", dtype=dtype, seed=seed)


def upcast_model(name):
    """An fp32 CPU model carrying the bf16 model's weights upcast."""
    src = cpu_model(name)
    m = LlamaModel(config(name), device="cpu", dtype=torch.float32, seed=SEED)
    m.embed, m.lm_head = src.embed.float(), src.lm_head.float()
    m.final_norm = src.final_norm.float()
    for a, b in zip(m.layers, src.layers):
        for k in ("wqkv", "wo", "wgate_up", "wdown", "attn_norm",
                  "mlp_norm"):
            setattr(a, k, getattr(b, k).float())
        a.bqkv = b.bqkv.float() if b.bqkv is not None else None
    return m


def case_tokens(name, tag, lens):
    """Seeded token lists, one per length."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(f"{name}/{tag}"))
    g = torch.Generator().manual_seed(seed)
    V = config(name).vocab
    return [torch.randint(0, V, (n,), generator=g).tolist() for n in lens]


# ---------------------------------------------------------------------------
# fp64 oracle


class Obs:
    """Observables of a set of sequences: logits[i] [n_i, V], K[i] and V[i]
    [L, n_i, KVH * 128] (K rotated)."""

    def __init__(self, logits, K, V):
        self.logits, self.K, self.V = logits, K, V


def _d(t):
    return t.detach().cpu().double()


def _rms_unit(x, eps, tiles=None):
    """x * rsqrt(mean(x^2) + eps); `tiles` (a mutant) sums the squares of
    only the first `tiles` 32-column tiles, as a consumer GEMM does that is
    handed too small a partial count."""
    H = x.shape[-1]
    sq = x * x
    if tiles is not None:
        sq = sq[..., :32 * tiles]
    return x * torch.rsqrt(sq.sum(-1, keepdim=True) / H + eps)


def oracle_forward(model, seqs, mut=None):
    """Dense fp64 forward of whole token sequences -> Obs (fp64).

    mut (tests only) plants one wiring fault:
      rope_pos   f(seq index, positions) -> positions used by RoPE
      drop_res   layer whose attention residual add is dropped
      rstd_tiles (layer, tiles): that layer's mlp norm sums `tiles` tiles
      bias_order the qkv bias is added in this (wrong) element order
      window     overrides cfg.sliding_window
      no_self    (seq index, position): that query misses its own key
    """
    mut = mut or {}
    cfg = model.cfg
    nl, nkl, eps = cfg.n_heads, cfg.n_kv_heads, cfg.norm_eps
    window = mut.get("window", cfg.sliding_window)
    cos, sin = model.rope_cos.cpu(), model.rope_sin.cpu()
    embed, lm = _d(model.embed), _d(model.lm_head)
    out_l, out_k, out_v = [], [], []
    for si, toks in enumerate(seqs):
        n = len(toks)
        pos = torch.arange(n)
        rpos = mut["rope_pos"](si, pos) if "rope_pos" in mut else pos
        vis = None
        if "no_self" in mut and mut["no_self"][0] == si:
            vis = ao.visible(pos.tolist(), n, window, n)
            p = mut["no_self"][1]
            vis[p, p] = False
        x = embed[torch.tensor(toks)]
        Ks, Vs = [], []
        for li, l in enumerate(model.layers):
            h = x
            y = (_rms_unit(h, eps) * _d(l.attn_norm)) @ _d(l.wqkv).t()
            if l.bqkv is not None:
                b = _d(l.bqkv)
                if "bias_order" in mut:
                    b = b[torch.tensor(mut["bias_order"])]
                y = y + b
            q = y[:, :nl * 128].reshape(n, nl, 128)
            k = y[:, nl * 128:(nl + nkl) * 128].reshape(n, nkl, 128)
            v = y[:, (nl + nkl) * 128:].reshape(n, nkl, 128)
            q = fo.rope_oracle(q, rpos, cos, sin)
            k = fo.rope_oracle(k, rpos, cos, sin)
            Ks.append(k.reshape(n, -1))
            Vs.append(v.reshape(n, -1))
            a = ao.attention_oracle(q, k, v, pos.tolist(), n, window,
                                    vis=vis)[0]
            o = a.reshape(n, -1) @ _d(l.wo).t()
            x = o if mut.get("drop_res") == li else o + h
            h = x
            tiles = mut["rstd_tiles"][1] \
                if mut.get("rstd_tiles", (None,))[0] == li else None
            gu = (_rms_unit(h, eps, tiles) * _d(l.mlp_norm)) \
                @ _d(l.wgate_up).t()
            x = h + fo.swiglu_oracle(gu) @ _d(l.wdown).t()
        out_l.append((_rms_unit(x, eps) * _d(model.final_norm)) @ lm.t())
        out_k.append(torch.stack(Ks))
        out_v.append(torch.stack(Vs))
    return Obs(out_l, out_k, out_v)


# ---------------------------------------------------------------------------
# reference run and the second emulation


def _prefill_meta(slot, n, window, dev="cpu"):
    return AttnMeta(
        mode="prefill",
        slot_ids=torch.tensor([slot], dtype=torch.int32, device=dev),
        seq_lens=torch.tensor([n], dtype=torch.int32, device=dev),
        cu_q=torch.tensor([0, n], dtype=torch.int32, device=dev),
        logits_idx=None, max_q=n, max_kv=n, window=window)


def cache_rows(kv, slot, n):
    """(K, V) [L, n, KVH * 128] of a slot, gathered through the page table."""
    L = kv.k_pool.shape[0]
    ks, vs = [], []
    for li in range(L):
        k, v = _gather_kv(kv, li, slot, n)
        ks.append(k.reshape(n, -1))
        vs.append(v.reshape(n, -1))
    return torch.stack(ks).cpu(), torch.stack(vs).cpu()


def reference_run(model, seqs):
    """Teacher-forced run of a CPU model through ops/reference.py: one
    prefill per sequence over the whole token list, logits at every
    position -> Obs in the model's dtype."""
    cfg = model.cfg
    pages = sum((len(s) + PAGE - 1) // PAGE for s in seqs)
    kv = PagedKVCache.for_model(
        cfg, n_pages=pages, max_slots=len(seqs),
        max_ctx=max(len(s) for s in seqs), device="cpu", dtype=model.dtype)
    L, K, V = [], [], []
    for toks in seqs:
        n = len(toks)
        slot = kv.alloc_slot()
        kv.ensure(slot, n)
        L.append(model.forward(
            torch.tensor(toks, dtype=torch.int32),
            torch.arange(n, dtype=torch.int32), kv,
            torch.full((n,), slot, dtype=torch.int32),
            _prefill_meta(slot, n, cfg.sliding_window)))
        k, v = cache_rows(kv, slot, n)
        K.append(k)
        V.append(v)
    return Obs(L, K, V)


def emulate_chain(model, seqs):
    """A second, independent bf16-staged emulation: it rounds to bf16 at the
    FUSED CHAIN's points only (residual stream, q/k/v, attention output,
    activation, logits; never the normed activation or gate_up),
    accumulates in fp32 and rounds P to bf16 in 32-row prefill tiles
    (attn_oracle.emulate_prefill)."""
    cfg = model.cfg
    nl, nkl, eps, H = cfg.n_heads, cfg.n_kv_heads, cfg.norm_eps, cfg.hidden
    cos, sin = model.rope_cos, model.rope_sin
    bf = torch.bfloat16

    def rstd(y):
        return torch.rsqrt((y * y).sum(-1, keepdim=True) / H + eps)

    out_l, out_k, out_v = [], [], []
    for toks in seqs:
        n = len(toks)
        pos = torch.arange(n)
        res = model.embed[torch.tensor(toks)].to(bf)
        r = rstd(res.float())
        Ks, Vs = [], []
        for l in model.layers:
            y = (res.float() @ l.wqkv.float().t()) * r
            if l.bqkv is not None:
                y = y + l.bqkv.float()
            q = y[:, :nl * 128].reshape(n, nl, 128)
            k = y[:, nl * 128:(nl + nkl) * 128].reshape(n, nkl, 128)
            v = y[:, (nl + nkl) * 128:].reshape(n, nkl, 128).to(bf)
            q = eo.emulate_rope(q, pos, cos, sin).to(bf)
            k = eo.emulate_rope(k, pos, cos, sin).to(bf)
            Ks.append(k.reshape(n, -1))
            Vs.append(v.reshape(n, -1))
            a = ao.emulate_prefill(q, k, v, 0, cfg.sliding_window)
            y = a.reshape(n, -1).float() @ l.wo.float().t() + res.float()
            r, res = rstd(y), y.to(bf)
            gu = (res.float() @ l.wgate_up.float().t()) * r
            F = gu.shape[1] // 2
            act = (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]).to(bf)
            y = act.float() @ l.wdown.float().t() + res.float()
            r, res = rstd(y), y.to(bf)
        out_l.append(((res.float() @ model.lm_head.float().t()) * r).to(bf))
        out_k.append(torch.stack(Ks))
        out_v.append(torch.stack(Vs))
    return Obs(out_l, out_k, out_v)


# ---------------------------------------------------------------------------
# metrics and budgets


def row_metrics(got, truth):
    """(rel, mx) per row of [..., width] tensors; NaN where got is not
    finite, which fails every comparison."""
    g, t = _d(got), _d(truth)
    assert g.shape == t.shape, f"shape {tuple(g.shape)} vs {tuple(t.shape)}"
    err = g - t
    rel = err.norm(dim=-1) / t.norm(dim=-1)
    mx = err.abs().amax(dim=-1) / t.pow(2).mean(dim=-1).sqrt()
    return rel, mx


class Budget:
    """2 x the reference run's worst rel and mx, per observable class:
    "logits", ("K", layer), ("V", layer)."""

    FACTOR = 2.0

    def __init__(self, ref, truth):
        self.lim, self.worst = {}, {}
        n_layers = truth.K[0].shape[0]
        self._add("logits", ref.logits, truth.logits)
        for li in range(n_layers):
            self._add(("K", li), [k[li] for k in ref.K],
                      [k[li] for k in truth.K])
            self._add(("V", li), [v[li] for v in ref.V],
                      [v[li] for v in truth.V])

    def _add(self, key, got, truth):
        rel, mx = zip(*(row_metrics(g, t) for g, t in zip(got, truth)))
        rel, mx = float(torch.cat(rel).max()), float(torch.cat(mx).max())
        assert math.isfinite(rel) and math.isfinite(mx) and rel > 0
        self.lim[key] = (self.FACTOR * rel, self.FACTOR * mx)

    def fresh(self):
        """The same limits with an empty record of worst ratios."""
        b = Budget.__new__(Budget)
        b.lim, b.worst = self.lim, {}
        return b

    @property
    def logits_mx(self):
        return self.lim["logits"][1]

    def ratio(self, key, got, truth):
        """Worst error / budget of some rows (inf on a non-finite row);
        remembered per key for the report."""
        rel, mx = row_metrics(got, truth)
        r = torch.maximum(rel / self.lim[key][0], mx / self.lim[key][1])
        r = float(torch.nan_to_num(r, nan=float("inf")).max()) \
            if r.numel() else 0.0
        self.worst[key] = max(self.worst.get(key, 0.0), r)
        return r

    def hold(self, key, got, truth, what=""):
        r = self.ratio(key, got, truth)
        assert r <= 1.0, f"{what} {key}: {r:.2f} x budget " \
                         f"(rel, mx <= {self.lim[key]})"
        return r

    def hold_obs(self, got, truth, what=""):
        """A whole Obs against the oracle; returns {key: ratio}."""
        self.hold("logits", torch.cat([_d(x) for x in got.logits]),
                  torch.cat(truth.logits), what)
        for li in range(truth.K[0].shape[0]):
            self.hold(("K", li), torch.cat([_d(k[li]) for k in got.K]),
                      torch.cat([k[li] for k in truth.K]), what)
            self.hold(("V", li), torch.cat([_d(v[li]) for v in got.V]),
                      torch.cat([v[li] for v in truth.V]), what)
        return dict(self.worst)

    def report(self):
        """(worst logits ratio, worst K/V ratio per layer)."""
        kv = {}
        for key, r in self.worst.items():
            if key != "logits":
                kv[key[1]] = max(kv.get(key[1], 0.0), r)
        return self.worst.get("logits", 0.0), [kv[i] for i in sorted(kv)]


def truth_and_budget(model, seqs):
    """(oracle Obs, Budget) of a CPU bf16 model at the given full token
    sequences (teacher forcing: pass what a run consumed and produced)."""
    truth = oracle_forward(model, seqs)
    return truth, Budget(reference_run(model, seqs), truth)


@functools.lru_cache(maxsize=None)
def truth_of(name, tag, lens):
    """(token lists, oracle Obs, Budget) of a case: computed once, shared
    and never modified."""
    seqs = case_tokens(name, tag, lens)
    return (seqs,) + truth_and_budget(cpu_model(name), seqs)


# ---------------------------------------------------------------------------
# trajectory check


def greedy_ok(L, tok, mx_budget):
    """Token `tok` was produced greedily after a prefix whose fp64 logits
    row is L: it must lie within gamma = 2 mx_budget rms(L) of the best."""
    L = _d(L)
    gamma = 2.0 * mx_budget * float(L.pow(2).mean().sqrt())
    return float(L[tok]) >= float(L.max()) - gamma


def gumbel_margin(L, T, seed, ctr):
    """fp64 scores L / T + g(u) of the in-graph Gumbel tail."""
    L = _d(L).numpy()
    u = eo.hash_u01(seed, ctr, np.arange(L.shape[0], dtype=np.int64))
    return L / T - np.log(-np.log(u.astype(np.float64)))


def gumbel_ok(L, tok, T, seed, ctr, mx_budget):
    """The sampled token's score is within gamma / T + GUMBEL_GAMMA of the
    best; also returns the oracle's best-to-runner-up margin minus that
    tolerance (> 0: the decision is unambiguous)."""
    s = gumbel_margin(L, T, seed, ctr)
    Ld = _d(L)
    tol = 2.0 * mx_budget * float(Ld.pow(2).mean().sqrt()) / T \
        + eo.GUMBEL_GAMMA
    top = np.sort(s)[-2:]
    return bool(s[tok] >= top[1] - tol), float(top[1] - top[0] - tol)


# ---------------------------------------------------------------------------
# pool helpers and the forward-level rig


def owned_mask(kv, lens_by_slot):
    """[n_pages, page] bool: the (page, offset) rows that slots own at the
    given lengths (ownership from kv._slot_pages)."""
    mask = torch.zeros(kv.n_pages, kv.page_size, dtype=torch.bool)
    for slot, n in lens_by_slot.items():
        pages = kv._slot_pages[slot]
        for p in range(n):
            mask[pages[p // kv.page_size], p % kv.page_size] = True
    return mask


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def assert_unowned_kept(kv, before, lens_by_slot, what=""):
    """Every pool element outside the owned rows keeps its bits.
    before = (k_pool bits, v_pool bits) from snapshot()."""
    free = ~owned_mask(kv, lens_by_slot)
    for nm, pool, was in (("k", kv.k_pool, before[0]),
                          ("v", kv.v_pool, before[1])):
        moved = (_bits(pool) != was).any(dim=-1)       # [L, P, KVH, page]
        bad = moved & free[None, :, None, :]
        assert not bool(bad.any()), \
            f"{what}: {nm}_pool changed outside the owned rows at " \
            f"(layer, page, head, offset) {bad.nonzero()[0].tolist()}"


def snapshot(kv):
    return _bits(kv.k_pool), _bits(kv.v_pool)


def scramble(kv, seed=0):
    """Make a fresh cache adversarial like attn_oracle.build_pool: slots
    and pages are handed out in a seeded shuffled order (never slots
    0, 1, 2, ...; page ids not ascending), unowned page-table entries point
    at a spare page nobody owns, and both pools hold elem_oracle's seeded
    finite pattern (distinct rows, all layers)."""
    g = torch.Generator().manual_seed(5000 + seed)
    assert not any(kv._slot_pages) and kv.n_pages >= 4
    while True:
        slots = torch.randperm(kv.max_slots, generator=g).tolist()
        if slots[-1] != 0:
            break
    pages = torch.randperm(kv.n_pages, generator=g).tolist()
    if pages[-1] < pages[-2]:          # the first two handed out descend
        pages[-1], pages[-2] = pages[-2], pages[-1]
    spare = pages.pop(0)
    kv._free_slots[:] = slots
    kv._free_pages[:] = pages
    kv.page_table.fill_(spare)
    kv.k_pool.copy_(eo._pattern(kv.k_pool.shape, 2 * seed + 21))
    kv.v_pool.copy_(eo._pattern(kv.v_pool.shape, 2 * seed + 22))
    return spare


class Rig:
    """A model, a scrambled cache and token sequences; drives
    LlamaModel.forward directly (no engine) and checks what it left."""

    def __init__(self, model, seqs, device, seed=0, max_slots=80):
        cfg = model.cfg
        self.model, self.seqs, self.dev = model, seqs, device
        pages = sum((len(s) + PAGE - 1) // PAGE for s in seqs) + 5
        self.kv = PagedKVCache.for_model(
            cfg, n_pages=pages, max_slots=max_slots, max_ctx=MAX_CTX,
            device=device, dtype=torch.bfloat16)
        scramble(self.kv, seed)
        self.slots = [self.kv.alloc_slot() for _ in seqs]
        assert self.slots != list(range(len(seqs)))
        self.before = snapshot(self.kv)
        self.done = [0] * len(seqs)        # tokens of each sequence in KV

    def forward(self, parts, mode, fused=False, logits_idx=True,
                capture=False, order=None):
        """One forward over parts [(seq, start, end)] (decode rows first
        in "mixed").  Returns (logits, [(seq, position)] per logits row)."""
        kv, dev = self.kv, self.dev
        if order is not None:
            parts = [parts[i] for i in order]
        tok, pos, slot, rows = [], [], [], []
        for s, a, b in parts:
            assert a == self.done[s]
            kv.ensure(self.slots[s], b)
            self.done[s] = b
            tok += self.seqs[s][a:b]
            pos += range(a, b)
            slot += [self.slots[s]] * (b - a)
            rows += [(s, b - 1)] if logits_idx else \
                [(s, p) for p in range(a, b)]
        cu = [0]
        for s, a, b in parts:
            cu.append(cu[-1] + b - a)
        lens = [b for _, _, b in parts]
        it = lambda x, dt=torch.int32: torch.tensor(x, dtype=dt, device=dev)
        meta = AttnMeta(
            mode=mode, slot_ids=it([self.slots[s] for s, _, _ in parts]),
            seq_lens=it(lens), cu_q=it(cu),
            logits_idx=it([c - 1 for c in cu[1:]], torch.long)
            if logits_idx else None,
            max_q=max(b - a for _, a, b in parts),
            max_kv=kv.max_ctx if capture else max(lens),
            n_decode=sum(1 for _, a, b in parts if b - a == 1)
            if mode == "mixed" else 0,
            window=self.model.cfg.sliding_window)
        had = self.model.fused_chain
        assert had or not fused, "the model has no fused chain"
        self.model.fused_chain = fused
        try:
            logits = self.model.forward(it(tok), it(pos), kv, it(slot), meta)
        finally:
            self.model.fused_chain = had
        return logits, rows

    def restore(self, state):
        """Back to a saved (pool, done) state; pages stay allocated."""
        (k, v), done = state
        self.kv.k_pool.copy_(k.view(torch.bfloat16).to(self.dev))
        self.kv.v_pool.copy_(v.view(torch.bfloat16).to(self.dev))
        self.done = list(done)

    def save(self):
        return snapshot(self.kv), list(self.done)

    def check(self, truth, budget, logits, rows, what=""):
        """Logits rows and every live K/V row within budget, no NaN,
        nothing outside the owned rows touched."""
        assert torch.isfinite(logits).all(), f"{what}: non-finite logits"
        want = torch.stack([truth.logits[s][p] for s, p in rows])
        budget.hold("logits", logits, want, what)
        for s, n in enumerate(self.done):
            if n == 0:
                continue
            k, v = cache_rows(self.kv, self.slots[s], n)
            for li in range(k.shape[0]):
                budget.hold(("K", li), k[li], truth.K[s][li, :n],
                            f"{what} seq {s}")
                budget.hold(("V", li), v[li], truth.V[s][li, :n],
                            f"{what} seq {s}")
        assert_unowned_kept(
            self.kv, self.before,
            {self.slots[s]: n for s, n in enumerate(self.done)}, what)


# ---------------------------------------------------------------------------
# forward-level cases: (tag, sequence lengths); the schedules live in
# run_case so the CPU file can hold the second emulation to every budget
# the GPU file uses

DECODE_B = (1, 5, 32, 33, 64)
EDGE_CTX = (1, 15, 16, 17, 63, 64, 65)
EXACT_B = (5, 40)


def decode_ctx(B):
    """Ragged context lengths: the page and chunk edges first (B = 1 takes
    65, past a chunk), short ones after so a case stays small."""
    if B == 1:
        return (65,)
    c = list(EDGE_CTX)[:B]
    return tuple(c + [2 + (i * 5) % 11 for i in range(B - len(c))])


PREFILL_CASES = (("one120", (120,)), ("varlen", (1, 31, 33, 65)),
                 ("chunks", (39,)))
# three decode rows, one fresh chunk, one continued chunk (88 + 12): rows 0
# and 2 and the continued chunk sit past tiny-swa's window of 96
MIXED_LENS = (100, 65, 16, 9, 100)
MIXED_CONT = 88


def forward_cases():
    """Every (tag, lens) the GPU forward file derives a budget for."""
    cases = list(PREFILL_CASES) + [("mixed", MIXED_LENS)]
    cases += [(f"decode{B}", tuple(c + 1 for c in decode_ctx(B)))
              for B in sorted(set(DECODE_B + EXACT_B))]
    return cases
