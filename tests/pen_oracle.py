"""fp64 oracle of the logit penalties (repeat / presence / frequency,
llama.cpp order), a second naive implementation, the oracle's mutants and
the shared cases (tests/test_penalty_cpu.py proves them on the CPU,
tests/test_penalty_gpu.py applies them to the HIP kernel and the engine).

Semantics, per row b of a batch:
  L = lens[b] clamped to [0, max_ctx]: the length AFTER this step's append;
  tok[b] >= 0 is written to hist[slot[b], L-1] first (inactive rows too);
  a row is inactive when last_n == 0 or (rp == 1, pp == 0, fp == 0);
  window = the last min(n, L) positions (n < 0: all L), ids outside [0, V)
  ignored; for every v with count c_v > 0
      x = x * rp if x <= 0 else x / rp;   x -= c_v * fp + pp.
The oracle sees the bf16 logits and the fp32 parameters upcast to double
and rounds nothing.  Everything here is numpy / torch on the CPU.
"""
import functools

import numpy as np
import torch

import fused_oracle as fo

MAX_CTX = 256
MAX_SLOTS = 64
VS = (64, 520, 4104, 128256)
BS = (1, 6, 33)
LENS = (1, 2, 63, 64, 65, 200, 256)
LAST_NS = (0, 1, 64, 65, -1, 10 ** 6)
INT_MAX = 2 ** 31 - 1

MUTANTS = ("lo_plus", "shift", "no_prompt", "cap", "rp_after", "no_append")
# `x < 0` for `x <= 0` is listed apart: see test_penalty_cpu.py
EQUIVALENT_MUTANTS = ("lt",)


def _np(t, dtype):
    return t.detach().cpu().numpy().astype(dtype)


def _window(h, sl, L, n, t, mut, prompt_len):
    """Window token ids (int64) of one active row; h already holds the
    append."""
    w = L if (n < 0 or n > L) else n
    lo, hi = L - w, L
    if mut == "lo_plus":                 # one token short at the old end
        lo = min(lo + 1, hi)
    elif mut == "shift":                 # off by one at the new end
        lo, hi = max(lo - 1, 0), max(hi - 1, 0)
    elif mut == "no_prompt":             # generated tokens only
        lo = min(max(lo, prompt_len), hi)
    return lo, hi


def oracle(logits, hist, slot, lens, tok, last_n, rp, pp, fp, mut=None,
           prompt_len=None):
    """(out fp64 [B, V], touched bool [B, V], hist after) as numpy arrays.
    mut names a deliberately wrong variant (MUTANTS)."""
    x = logits.detach().cpu().double().numpy().copy()
    B, V = x.shape
    h = _np(hist, np.int64).copy()
    max_ctx = h.shape[1]
    slot, lens, tok, last_n = (_np(a, np.int64)
                               for a in (slot, lens, tok, last_n))
    rp, pp, fp = (_np(a.float(), np.float64) for a in (rp, pp, fp))
    touched = np.zeros((B, V), dtype=bool)
    for b in range(B):
        sl, t, n = int(slot[b]), int(tok[b]), int(last_n[b])
        L = min(max(int(lens[b]), 0), max_ctx)
        stale = h[sl, L - 1] if L >= 1 else -1
        if t >= 0 and L >= 1:
            h[sl, L - 1] = t
        r, p, f = rp[b], pp[b], fp[b]
        if n == 0 or (r == 1.0 and p == 0.0 and f == 0.0):
            continue
        lo, hi = _window(h, sl, L, n, t, mut,
                         0 if prompt_len is None else int(prompt_len[b]))
        win = h[sl, lo:hi].copy()
        if mut == "no_append" and t >= 0 and hi == L and hi > lo:
            win[-1] = stale              # counts what the cell held before
        win = win[(win >= 0) & (win < V)]
        c = np.bincount(win, minlength=V)
        ids = np.nonzero(c)[0]
        cc = c[ids].astype(np.float64)
        if mut == "cap":
            cc = np.minimum(cc, 1.0)
        xv = x[b, ids]
        if mut == "rp_after":
            xv = xv - (cc * f + p)
            xv = np.where(xv <= 0, xv * r, xv / r)
        else:
            neg = (xv < 0) if mut == "lt" else (xv <= 0)
            xv = np.where(neg, xv * r, xv / r)
            xv = xv - (cc * f + p)
        x[b, ids] = xv
        touched[b, ids] = True
    return x, touched, h.astype(np.int32)


def naive(logits, hist, slot, lens, tok, last_n, rp, pp, fp):
    """The same contract as a plain Python loop over window positions with
    a dict of counts; shares no code with oracle()."""
    x = [[float(v) for v in row] for row in logits.detach().cpu().double()
         .tolist()]
    h = [list(r) for r in hist.tolist()]
    B, V = len(x), len(x[0])
    touched = [set() for _ in range(B)]
    for b in range(B):
        sl, L, t, n = int(slot[b]), int(lens[b]), int(tok[b]), int(last_n[b])
        L = 0 if L < 0 else (len(h[0]) if L > len(h[0]) else L)
        if t >= 0 and L >= 1:
            h[sl][L - 1] = t
        r = float(rp[b].float().double())
        p = float(pp[b].float().double())
        f = float(fp[b].float().double())
        if n == 0:
            continue
        if r == 1.0 and p == 0.0 and f == 0.0:
            continue
        start = 0 if n < 0 else max(0, L - n)
        counts = {}
        for i in range(start, L):
            v = h[sl][i]
            if 0 <= v < V:
                counts[v] = counts.get(v, 0) + 1
        for v, c in counts.items():
            val = x[b][v]
            val = val * r if val <= 0 else val / r
            val -= c * f + p
            x[b][v] = val
            touched[b].add(v)
    return x, touched, h


# ---------------------------------------------------------------------------
# cases


EXACT = dict(rp=(1.0, 2.0, 0.5), pp=(0.0, 1.0, -1.0), fp=(0.0, 1.0))
REAL = dict(rp=(1.1, 1.3, 0.8), pp=(0.0, 0.5, -0.7, 1.9),
            fp=(0.0, 0.5, -0.7, 1.9))


@functools.lru_cache(maxsize=None)
def make_case(V, B, tier, variant=0):
    """One batch.  Rows cycle through the window patterns, lengths, window
    sizes, append / no append and active / inactive, starting at an offset
    that differs between cases, so B = 1 cases see different rows.  Returns
    a dict of CPU tensors; "prompt_len" serves the prompt-excluded mutant
    only."""
    g = torch.Generator().manual_seed(
        9176 + V * 31 + B * 7 + (tier == "real") * 3 + variant * 1013)
    off = VS.index(V) * 5 + BS.index(B) * 3 + (tier == "real") + variant * 2

    def ri(lo, hi, shape):
        return torch.randint(lo, hi, shape, generator=g)

    # seeded garbage everywhere: in-range ids, ids just outside [0, V) and
    # INT_MAX, so a read outside the window or in another slot shows
    hist = ri(-3, V + 3, (MAX_SLOTS, MAX_CTX)).int()
    hist[ri(0, 7, hist.shape) == 0] = INT_MAX
    slot = torch.randperm(MAX_SLOTS, generator=g)[:B].int()
    if tier == "exact":
        logits = (ri(-16, 17, (B, V)) * 2).float().bfloat16()
        par = EXACT
    else:
        logits = (torch.randn((B, V), generator=g) * 2.0).bfloat16()
        par = REAL
    lens, tok, last_n, rp, pp, fp, plen = [], [], [], [], [], [], []
    for b in range(B):
        k = b + off
        L = LENS[k % len(LENS)]
        n = LAST_NS[(k // 2 + b) % len(LAST_NS)]
        sl = int(slot[b])
        pat = k % 4
        if pat == 0:      # distinct as far as V allows
            perm = torch.randperm(V, generator=g)
            row = perm[torch.arange(L) % V]
        elif pat == 1:    # one token up to 150 times: the adds share a cell
            row = ri(0, V, (L,))
            rep = min(L, 150)
            at = torch.randperm(L, generator=g)[:rep]
            row[at] = int(ri(0, V, (1,)))
        elif pat == 2:    # the first and the last id
            row = ri(0, V, (L,))
            row[ri(0, L, (max(1, L // 3),))] = 0
            row[ri(0, L, (max(1, L // 3),))] = V - 1
        else:             # ids that must be ignored, inside the window
            row = ri(0, V, (L,))
            bad = torch.tensor([-1, V, INT_MAX])
            row[ri(0, L, (min(L, 9),))] = bad[ri(0, 3, (min(L, 9),))]
        hist[sl, :L] = row.int()
        append = k % 3 != 2
        if append:
            # the cell the kernel writes holds garbage: reading it back
            # instead of taking tok counts the wrong token
            tok.append(int(row[L - 1]) if 0 <= int(row[L - 1]) < V
                       else int(ri(0, V, (1,))))
            hist[sl, L - 1] = int(ri(0, V, (1,))) if k % 2 else INT_MAX
        else:
            tok.append(-1)
        neutral = k % 5 == 4          # rp = 1, pp = 0, fp = 0: inactive
        if B == 1:                    # the only row is an active one
            neutral, n = False, LAST_NS[1 + off % 5]
        rp.append(1.0 if neutral else par["rp"][k % len(par["rp"])])
        pp.append(0.0 if neutral else par["pp"][(k // 3) % len(par["pp"])])
        fp.append(0.0 if neutral else par["fp"][(k // 2) % len(par["fp"])])
        if B == 1 and (rp[-1], pp[-1], fp[-1]) == (1.0, 0.0, 0.0):
            pp[-1] = par["pp"][1]
        lens.append(L)
        last_n.append(n)
        plen.append(L // 2)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)          # noqa: E731
    f32 = lambda a: torch.tensor(a, dtype=torch.float32)        # noqa: E731
    return dict(name=f"V{V}-B{B}-{tier}" + (f"-{variant}" if variant else ""),
                tier=tier, logits=logits, hist=hist, slot=slot,
                lens=i32(lens), tok=i32(tok), last_n=i32(last_n),
                rp=f32(rp), pp=f32(pp), fp=f32(fp), prompt_len=i32(plen))


ARGS = ("logits", "hist", "slot", "lens", "tok", "last_n", "rp", "pp", "fp")


def cases():
    """(V, B, tier) of every shared case; build with make_case(*key)."""
    return [(V, B, tier) for V in VS for B in BS
            for tier in ("exact", "real")]


def case_id(key):
    return f"V{key[0]}-B{key[1]}-{key[2]}"


@functools.lru_cache(maxsize=None)
def truth(key):
    """oracle() of a case, computed once and never modified."""
    c = make_case(*key)
    return oracle(*(c[a] for a in ARGS))


def active_rows(c):
    n, r, p, f = c["last_n"], c["rp"], c["pp"], c["fp"]
    return (n != 0) & ~((r == 1) & (p == 0) & (f == 0))


def appended_cells(c):
    """[(slot, position, token)] the op must write."""
    out = []
    for s, L, t in zip(c["slot"].tolist(), c["lens"].tolist(),
                       c["tok"].tolist()):
        L = min(max(L, 0), MAX_CTX)
        if t >= 0 and L >= 1:
            out.append((s, L - 1, t))
    return out


def check_against_oracle(key, got, hist_after, what):
    """The checks shared with the GPU file: exact tier bit for bit, real
    tier inside the bf16 budget on the touched elements and bit for bit on
    every other one; hist identical except at the appended cells.  Returns
    the worst real-tier ratio."""
    c = make_case(*key)
    x, touched, h = truth(key)
    want = torch.from_numpy(x)
    got = got.detach().cpu()
    assert torch.equal(hist_after.detach().cpu(), torch.from_numpy(h)), \
        f"{what}: hist differs"
    want_h = c["hist"].clone()
    for s, p, t in appended_cells(c):
        want_h[s, p] = t
    assert torch.equal(torch.from_numpy(h), want_h)
    worst = 0.0
    if key[2] == "exact":
        assert bool((want == want.round()).all()) \
            and float(want.abs().max()) < 256
        assert torch.equal(got, want.bfloat16()), f"{what}: exact tier"
        return worst
    m = torch.from_numpy(touched)
    assert torch.equal(got[~m], c["logits"][~m]), \
        f"{what}: an untouched logit changed"
    for b in range(key[1]):
        if m[b].any():
            worst = max(worst, fo.assert_bf16_close(
                got[b], want[b], f"{what} row {b}"))
    return worst
