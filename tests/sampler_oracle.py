"""fp64 oracle of the step that turns a logits row into a token: the per-row
temperature / top-k / top-p filter and the distribution a sampling path
draws from.  Pure numpy/torch on the CPU; no HIP.

Semantics (the project's documented ones):
  * T <= 0 is greedy: the lowest-index maximum.
  * top-k (0 or >= V: off) and top-p (>= 1: off) are independent masks over
    the same descending order of l / T.
  * top-p keeps rank j iff the FULL-vocabulary mass strictly before j is
    < top_p; rank 0 is always kept.
  * the kept probabilities are renormalised.

Equal logits make "which token is rank j" implementation-defined, so the
oracle speaks in VALUES: the kept set is the multiset of the n largest
values; a token is in the support iff its logit is >= the n-th largest.

Capture: a test replaces torch.multinomial by a `Capture`, which records the
probability matrix a path hands over and returns a planted column per row
(first non-zero, last non-zero, or a seeded interior non-zero column).  That
makes every host path deterministic, shows the distribution actually sampled
from, and checks the rank -> token gather: where the matrix row is sorted,
the returned token's logit must equal the oracle's value at the planted
rank; where it is in token order the token must be the planted column."""
import functools
import math

import numpy as np
import torch

import elem_oracle as eo

P_FLOOR = 2.0 ** -20            # floor of the per-element relative budget
# fp32 holds a softmax term down to 2^-126; below 2^-120 (six bits of room
# for the renormalisation and the subtraction of the maximum) a path may
# flush a probability to zero, and relative error means nothing
P_TINY = 2.0 ** -120
AMBIGUOUS_CAP = 0.02            # share of a case's rows that may be ambiguous

TEMPS = (1e-3, 0.7, 1.0, 1.3, 100.0)
TOP_PS = (1e-9, 0.1, 0.5, 0.9, 0.95, 1.0 - 2.0 ** -20, 1.0, 1.5)


def _f32(x):
    """A python scalar or 0-d tensor as the double value of its fp32."""
    if torch.is_tensor(x):
        x = x.item()
    return float(np.float32(x))


class Dist:
    """One row's filtered distribution.  greedy rows carry only `token`."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def filtered_distribution(row, T, top_k, top_p, mutant=None):
    """row: [V] bf16 (or float) tensor; T, top_p as the sampler sees them
    (fp32), top_k int.  Returns a Dist with
      raw    [V] the logits sorted descending (float64, exact)
      vals   [V] raw / T
      probs  [V] full-vocabulary probabilities of `vals`
      before [V] mass strictly before each rank
      n      kept count
      kept   [n] renormalised kept probabilities
    `mutant` names a deliberate mistake (tests only)."""
    l = row.detach().double().cpu().numpy()
    V = l.shape[0]
    T, top_p, top_k = _f32(T), _f32(top_p), int(top_k)
    if T <= 0:
        return Dist(greedy=True, token=int(np.argmax(l)), V=V)
    raw = np.sort(l)[::-1].copy()
    Tm = 1.0 if mutant == "temp_after_cut" else T
    vals = raw / Tm
    with np.errstate(invalid="ignore"):
        e = np.exp(vals - vals[0])
    if mutant == "mass_top256":
        probs = e / e[:256].sum()
    else:
        probs = e / e.sum()
    cum = np.cumsum(probs)
    before = cum - probs
    before[0] = 0.0
    k = V if (top_k <= 0 or top_k >= V) else top_k
    if mutant == "topk_off_by_one" and k < V:
        k -= 1
    keep = np.arange(V) < k
    if top_p < 1.0:
        keep &= (cum < top_p) if mutant == "cum_lt_p" else (before < top_p)
    if mutant != "rank0_not_forced":
        keep[0] = True
    n = int(keep.sum())
    assert n == 0 or keep[:n].all(), "kept ranks are a prefix"
    if mutant == "temp_after_cut":
        vals = raw / T
        with np.errstate(invalid="ignore"):
            e = np.exp(vals - vals[0])
        probs = e / e.sum()
    kept = probs[:n] / probs[:n].sum() if n else probs[:0]
    return Dist(greedy=False, V=V, raw=raw, vals=vals, probs=probs,
                before=before, n=n, kept=kept, k=k, top_p=top_p, T=T)


def naive_distribution(row, T, top_k, top_p):
    """The same semantics as a python loop over the sorted ranks; used only
    to cross-check filtered_distribution.  Returns (n, kept list)."""
    l = [float(x) for x in row.detach().double().cpu().tolist()]
    V = len(l)
    T, top_p, top_k = _f32(T), _f32(top_p), int(top_k)
    if T <= 0:
        best = 0
        for i in range(1, V):
            if l[i] > l[best]:
                best = i
        return best, None
    s = sorted((x / T for x in l), reverse=True)
    m = s[0]
    e = [math.exp(x - m) if x != -math.inf else 0.0 for x in s]
    Z = math.fsum(e)
    kept, mass = [], 0.0
    for j in range(V):
        in_k = top_k <= 0 or top_k >= V or j < top_k
        in_p = top_p >= 1.0 or mass < top_p
        if j > 0 and not (in_k and in_p):
            break
        kept.append(e[j] / Z)
        mass += e[j] / Z
    tot = math.fsum(kept)
    return len(kept), [x / tot for x in kept]


def boundary_margin(d):
    """Smallest |mass before rank j - top_p| over the ranks whose top-p
    decision can change the kept set: 1 <= j < k (rank 0 is forced; ranks
    from k on are cut by top-k whatever their mass).  inf when top-p is
    off or the row is greedy."""
    if d.greedy or d.top_p >= 1.0 or d.k <= 1:
        return math.inf
    return float(np.abs(d.before[1:d.k] - d.top_p).min())


def in_support(row, tok, T, top_k, top_p):
    """Exact on values: token `tok` of `row` may be produced under the
    filter.  Greedy rows: the lowest-index maximum only."""
    d = filtered_distribution(row, T, top_k, top_p)
    if d.greedy:
        return tok == d.token
    x = float(row[tok])
    return math.isfinite(x) and d.n > 0 and x >= d.raw[d.n - 1]


def class2_expected(cand, T, seed, ctr):
    """cand: [C] candidate values as the tail hands them to the Gumbel
    kernel (raw logits, -inf where filtered out).  The expected candidate
    is the fp64 argmax of v_c / T - log(-log(u(seed, ctr, c))) with the
    candidate RANK c as the hash's third key.  Returns (best, runner,
    gap); gap >= eo.GUMBEL_GAMMA must match exactly, else either."""
    v = np.asarray(cand, dtype=np.float64)
    u = eo.hash_u01(seed, ctr, np.arange(v.shape[0], dtype=np.int64))
    sc = v / _f32(T) - np.log(-np.log(u.astype(np.float64)))
    best = int(np.argmax(sc))
    rest = sc.copy()
    rest[best] = -np.inf
    runner = int(np.argmax(rest))
    gap = float(sc[best] - rest[runner]) if np.isfinite(rest[runner]) \
        else math.inf
    return best, runner, gap


def class2_gamma(cand, T):
    """elem_oracle's decision margin, which is 16 x the float32 error of a
    score of magnitude <= 30 (half an ulp there is 9.5e-7), scaled with
    the ulp where v / T is larger (T = 1e-3 gives scores in the
    thousands, whose float32 ulp alone is 2.4e-4)."""
    v = np.asarray(cand, dtype=np.float64)
    big = float(np.abs(v[np.isfinite(v)]).max()) / _f32(T)
    return eo.GUMBEL_GAMMA * max(1.0, big / 32.0)


def class2_ok(cand, T, seed, ctr, got):
    best, runner, gap = class2_expected(cand, T, seed, ctr)
    return got == best or (gap < class2_gamma(cand, T) and got == runner)


# ---------------------------------------------------------------------------
# capture


class Capture:
    """Stand-in for torch.multinomial."""

    def __init__(self, plant, seed=0):
        assert plant in ("first", "last", "interior")
        self.plant, self.calls = plant, []
        self._rng = np.random.RandomState(seed)

    def __call__(self, probs, num_samples=1, replacement=False, *,
                 generator=None, out=None):
        assert num_samples == 1 and probs.dim() == 2
        p = probs.detach().double().cpu().numpy()
        picks = []
        for r in p:
            nz = np.flatnonzero(r > 0)
            assert nz.size, "a row with no mass reached multinomial"
            if self.plant == "first":
                picks.append(int(nz[0]))
            elif self.plant == "last":
                picks.append(int(nz[-1]))
            else:
                picks.append(int(nz[self._rng.randint(nz.size)]))
        self.calls.append((p, picks))
        return torch.tensor(picks, dtype=torch.long,
                            device=probs.device).unsqueeze(1)


def run_captured(sample_fn, case, plant, device="cpu"):
    """Runs sample_fn on the case with torch.multinomial replaced.  Returns
    (tokens list, {row: (probability row, planted column)}, widths)."""
    cap = Capture(plant, seed=len(case["name"]))
    real = torch.multinomial
    torch.multinomial = cap
    try:
        a = case_args(case, device)
        toks = sample_fn(a[0], a[1], a[2], a[3], None)
    finally:
        torch.multinomial = real
    toks = [int(t) for t in toks.tolist()]
    B = case["logits"].shape[0]
    stoch = [r for r in range(B) if _f32(case["T"][r]) > 0]
    seen, widths = {}, []
    for p, picks in cap.calls:
        rows = list(range(B)) if p.shape[0] == B else stoch
        assert p.shape[0] == len(rows), (p.shape, B, len(stoch))
        widths.append(p.shape[1])
        for i, r in enumerate(rows):
            assert r not in seen, "a row was sampled twice"
            seen[r] = (p[i], picks[i])
    return toks, seen, widths


def check_row(case, r, tok, obs, budget, gamma_p, mutant=None, T0=False):
    """One row of a captured run against the oracle.  Returns (error /
    budget ratio, ambiguous flag); raises AssertionError on a miss.
    obs: (probability row, planted column) or None for a greedy row."""
    row = case["logits"][r]
    src = 0 if T0 else r
    d = filtered_distribution(row, case["T"][src], case["top_k"][src],
                              case["top_p"][src], mutant=mutant)
    what = f"{case['name']} row {r}"
    if d.greedy:
        assert tok == d.token, \
            f"{what}: greedy token {tok}, lowest-index argmax {d.token}"
        return 0.0, False
    assert obs is not None, f"{what}: no distribution reached multinomial"
    p, c = obs
    # a fast path hands greedy rows over too; only stochastic rows count
    srt = np.sort(p)[::-1]
    n_seen = int((srt > 0).sum())
    amb = boundary_margin(d) < gamma_p
    counts = (d.n - 1, d.n, d.n + 1) if amb else (d.n,)
    err = None
    for n in counts:
        if n < 1 or n > d.V or n_seen > n:
            continue
        kept = d.probs[:n] / d.probs[:n].sum()
        # ranks that vanished must be ones fp32 may flush to zero
        if n_seen < n and kept[n_seen:].max() >= P_TINY:
            continue
        big = kept[:n_seen] >= P_TINY
        e = np.abs(srt[:n_seen] - kept[:n_seen])
        if (e[~big] > 2 * P_TINY).any():
            continue
        rel = float((e[big] / kept[:n_seen][big]).max()) if big.any() else 0.0
        if err is None or rel < err:
            err, n_used = rel, n
    assert err is not None, \
        f"{what}: {n_seen} non-zero probabilities, oracle keeps {d.n}" \
        f" (margin {boundary_margin(d):.3g}, gamma_p {gamma_p:.3g})"
    assert err <= budget, \
        f"{what}: kept probabilities off by {err:.3g} > budget {budget:.3g}"
    # planted pick -> token
    x = float(row[tok])
    if (np.diff(p) <= 0).all():
        assert x == d.raw[c], \
            f"{what}: planted rank {c} has value {d.raw[c]}, token {tok}" \
            f" has {x}"
    else:
        assert tok == c, f"{what}: planted column {c} came back as {tok}"
    assert math.isfinite(x) and x >= d.raw[n_used - 1], \
        f"{what}: token {tok} outside the support"
    return err / budget, amb


# ---------------------------------------------------------------------------
# cases


def _randn_bf16(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, V, generator=g) * 2.0).bfloat16()


def _tie_at(row, ranks):
    """Gives the tokens at the listed descending ranks the value of the
    first listed rank."""
    order = torch.argsort(row.float(), descending=True, stable=True)
    for r in ranks[1:]:
        row[order[r]] = row[order[ranks[0]]]


def _case(name, logits, T, top_k, top_p, scalar=False):
    B = logits.shape[0]
    assert len(T) == len(top_k) == len(top_p) == B
    return dict(name=name, logits=logits, T=list(T), top_k=list(top_k),
                top_p=list(top_p), scalar=scalar)


@functools.lru_cache(maxsize=None)
def cases():
    """The shared case list; built once, never modified."""
    out = []
    V = 64
    out.append(_case(
        "v64-mixed", _randn_bf16(8, V, 11),
        [1.3, 1.0, 0.0, 0.7, 100.0, 1e-3, -1.0, 1.0],
        [0, 1, 5, 2, V - 1, V, 0, V + 7],
        [1.0 - 2.0 ** -20, 0.5, 0.5, 0.9, 0.95, 0.1, 0.9, 1.5]))
    V = 520
    lg = _randn_bf16(1, V, 12).expand(8, V).clone()
    out.append(_case("v520-topk-differs", lg, [1.0] * 8,
                     [1, 2, 5, 255, 256, 257, V - 1, 0], [0.9] * 8))
    lg = _randn_bf16(1, V, 13).expand(9, V).clone()
    # top_p = 0 is no request's value (the engine maps it to "off"); the
    # sampler itself must still keep rank 0
    out.append(_case("v520-topp-differs", lg, [1.3] * 9, [0] * 9,
                     list(TOP_PS) + [0.0]))
    # the same two batches inside 0 < top_k <= 256, so that hip.sample's
    # fast path and the class-2 tail see them: one logits row, and only
    # top_k (top_p off) or only top_p (top_k fixed) differs between rows
    lg = _randn_bf16(1, V, 25).expand(6, V).clone()
    out.append(_case("v520-topk-capped", lg, [1.0] * 6,
                     [1, 2, 5, 40, 255, 256], [1.0] * 6))
    lg = _randn_bf16(1, V, 26).expand(8, V).clone()
    out.append(_case("v520-topp-capped", lg, [1.0] * 8, [256] * 8,
                     list(TOP_PS)))
    out.append(_case("v520-temp-only", _randn_bf16(5, V, 14),
                     [0.7, 1.0, 1.3, 100.0, 1e-3], [0, V, V + 7, 0, 0],
                     [1.0, 1.5, 1.0, 1.0, 1.5]))
    out.append(_case("v520-scalar", _randn_bf16(3, V, 15), [0.7] * 3,
                     [5] * 3, [0.9] * 3, scalar=True))
    out.append(_case("v64-scalar-temp", _randn_bf16(3, 64, 16), [1.3] * 3,
                     [0] * 3, [1.0] * 3, scalar=True))
    V = 4104
    out.append(_case(
        "v4104-fast", _randn_bf16(8, V, 17),
        [1e-3, 0.7, 1.0, 1.3, 100.0, 0.7, 1.0, 1.3],
        [5, 255, 256, 2, 256, 1, 40, 255],
        [0.9, 0.95, 0.5, 1.0 - 2.0 ** -20, 1.5, 0.1, 1e-9, 1.0]))
    lg = _randn_bf16(6, V, 18)
    lg[1, 7] = lg[1, 4000] = lg[1, 8] = 12.0       # greedy T = 0, tied maxima
    lg[4, V - 1] = lg[4, 3] = 12.0                 # greedy T = -1
    out.append(_case("v4104-fast-greedy", lg,
                     [0.7, 0.0, 1.0, 1.3, -1.0, 1.0],
                     [5, 0, 256, 40, 0, 2],
                     [0.9, 1.0, 0.95, 0.5, 0.5, 1.0]))
    out.append(_tie_case("v4104-ties", V, 19))
    lg = _randn_bf16(4, V, 20)
    lg[0] = (lg[0].float() / 2).bfloat16()         # N(0, 1): a wide nucleus
    out.append(_case("v4104-nucleus", lg,
                     [1.0, 0.7, 1.3, 1.0], [0, 0, 257, 0],
                     [0.5, 1.0, 0.9, 0.1]))
    out.append(_tie_case("v520-ties", 520, 21))
    # T = 1e-3 with the five best one bf16 step (2^-6) apart: their
    # probabilities fall by e^-15.6 per rank, all above P_TINY, while the
    # fp32 running mass is 1.0 from rank 2 on.  top_p = 1.0 is "off", not
    # a cut at 1.0: all five stay
    lg = _randn_bf16(6, 520, 24).float().clamp(max=3.5)
    for j in range(5):
        lg[:, 37 + 11 * j] = 3.984375 - j * 0.015625
    out.append(_case("v520-cold", lg.bfloat16(),
                     [1e-3, 1e-3, 1e-3, 1e-3, 0.7, 1e-3],
                     [5, 5, 5, 256, 5, 2],
                     [1.0, 1.5, 0.9, 1.0, 1.0, 0.5]))
    V = 128256
    out.append(_case("v128256-fast", _randn_bf16(6, V, 22),
                     [0.7, 1.0, 1.3, 1e-3, 100.0, 1.0],
                     [5, 256, 255, 2, 256, 40],
                     [0.9, 0.5, 0.95, 1.0, 0.1, 1.5]))
    lg = _randn_bf16(5, V, 23)
    lg[4, 5] = lg[4, V - 1] = 12.0
    # at this V the fp32 cumsum error (1e-5) exceeds the spacing of the
    # masses deep in the row, so a top-p cut is placed near the head only
    out.append(_case("v128256-sort", lg, [0.7, 0.7, 1.3, 1.0, 0.0],
                     [0, V - 1, 257, V + 7, 0],
                     [0.1, 1.5, 0.95, 1.0, 0.9]))
    return tuple(out)


def _tie_case(name, V, seed):
    """Every row has 0 < top_k <= 256 (so the case also serves the class-2
    tail): ties across the top-k boundary, at the maximum, a flat row, a
    row with one finite entry, a row with a block of -inf."""
    lg = _randn_bf16(8, V, seed)
    _tie_at(lg[0], (4, 5, 6))                # k = 5: ranks k-1, k, k+1
    _tie_at(lg[1], (255, 256, 257))          # k = 256
    _tie_at(lg[2], (0, 1, 2))                # ties at the maximum
    lg[3] = 0.5                              # flat
    lg[4] = float("-inf")
    lg[4, V // 3] = 1.25                     # one finite entry
    lg[5, 100:100 + V // 2] = float("-inf")  # a block of -inf
    lg[6, 9] = lg[6, V - 2] = 12.0           # greedy, tied maxima
    _tie_at(lg[7], (1, 2, 3))                # k = 2
    return _case(name, lg,
                 [1.0, 0.7, 1.3, 1.0, 0.7, 1.0, 0.0, 1.0],
                 [5, 256, 3, 5, 40, 255, 7, 2],
                 [1.0, 0.95, 0.9, 0.9, 0.9, 0.95, 0.9, 1.5])


def case(name):
    for c in cases():
        if c["name"] == name:
            return c
    raise KeyError(name)


def case_names():
    return [c["name"] for c in cases()]


def fast_path(c):
    """hip.sample takes its top-256 path: every stochastic row carries
    0 < top_k <= min(256, V)."""
    C = min(256, c["logits"].shape[1])
    return all(_f32(t) <= 0 or 0 < k <= C
               for t, k in zip(c["T"], c["top_k"]))


def case_args(c, device="cpu"):
    """(logits, temperature, top_k, top_p) as the samplers take them."""
    lg = c["logits"].to(device)
    if c["scalar"]:
        return lg, c["T"][0], c["top_k"][0], c["top_p"][0]
    return (lg, torch.tensor(c["T"], dtype=torch.float32, device=device),
            torch.tensor(c["top_k"], dtype=torch.long, device=device),
            torch.tensor(c["top_p"], dtype=torch.float32, device=device))


# ---------------------------------------------------------------------------
# measured budgets


@functools.lru_cache(maxsize=None)
def budget(name):
    """(relative budget, gamma_p, reference error, cumsum error) of a case,
    measured on the fp32 CPU reference: 4 x its worst relative error of a
    kept probability (floored at 2^-20), and 4 x its worst fp32 cumsum
    error."""
    from ollamamq_amd.ops import reference as ref
    c = case(name)
    toks, seen, _ = run_captured(ref.sample, c, "first")
    worst = 0.0
    for r, (p, _) in seen.items():
        d = filtered_distribution(c["logits"][r], c["T"][r], c["top_k"][r],
                                  c["top_p"][r])
        srt = np.sort(p)[::-1]
        m = min(int((srt > 0).sum()), d.n)
        kept = d.kept[:m]
        big = kept >= P_TINY
        if big.any():
            worst = max(worst, float(
                (np.abs(srt[:m] - kept)[big] / kept[big]).max()))
    cum_err = 0.0
    for r in range(c["logits"].shape[0]):
        T = _f32(c["T"][r])
        if T <= 0:
            continue
        l32 = c["logits"][r].float() / torch.tensor(T, dtype=torch.float32)
        sp = torch.softmax(l32.sort(descending=True).values, dim=-1)
        cum32 = sp.cumsum(-1).double().numpy()
        d = filtered_distribution(c["logits"][r], T, 0, 1.0)
        cum_err = max(cum_err, float(np.abs(
            cum32 - np.cumsum(d.probs)).max()))
    return max(4.0 * worst, P_FLOOR), 4.0 * cum_err, worst, cum_err
