"""The sampling paths on the GPU held to the fp64 distribution oracle
(tests/sampler_oracle.py): hip.sample (top-256 fast path and sort fallback)
through the multinomial capture, the engine's class-2 tail run eagerly with
the Gumbel kernel's input recorded, and the engine's default host path
(class 3) with every produced token checked against the support computed
from the logits row its step recorded."""
import numpy as np
import pytest
import torch

import elem_oracle as eo
import sampler_oracle as so
from test_engine_oracle_gpu import Tap, _check, _drive, _engine, _submit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


# ---------------------------------------------------------------------------
# hip.sample


@pytest.mark.parametrize("name", so.case_names())
def test_hip_sample_holds_the_oracle(name):
    hip = _hip()
    c = so.case(name)
    B, V = c["logits"].shape
    bud, gamma_p, _, _ = so.budget(name)
    n_stoch = sum(so._f32(t) > 0 for t in c["T"])
    worst = 0.0
    for plant in ("first", "last", "interior"):
        toks, seen, widths = so.run_captured(hip.sample, c, plant, DEV)
        if so.fast_path(c):
            # evidence that the top-256 path ran
            assert widths == [min(256, V)], widths
        else:
            assert widths == [V], widths
        amb = 0
        for r in range(B):
            ratio, a = so.check_row(c, r, toks[r], seen.get(r), bud, gamma_p)
            worst, amb = max(worst, ratio), amb + a
        assert amb <= so.AMBIGUOUS_CAP * n_stoch, (name, amb)
    group = "fast" if so.fast_path(c) else "sort"
    print(f"RATIO hip.sample-{group} {name} {worst:.3f} "
          f"(budget {bud:.3e})")


def test_hip_sample_all_greedy_ties():
    """The all-greedy path on rows with planted equal maxima."""
    hip = _hip()
    for name in ("v4104-fast-greedy", "v520-ties"):
        c = so.case(name)
        lg = c["logits"].to(DEV)
        out = hip.sample(lg, 0.0, 0, 1.0, None).tolist()
        want = np.argmax(c["logits"].double().numpy(), axis=1).tolist()
        assert out == want


# ---------------------------------------------------------------------------
# class-2 tail, eagerly

TAIL_SEEDS = (0, -1, 2 ** 63 - 1, -2 ** 63)
TAIL_CTRS = (1, 4095)
# (case, rows): every stochastic row has 0 < top_k <= 256
TAIL_CASES = (
    ("v520-ties", (0, 1, 2, 3, 4, 5)),
    ("v520-ties", (6,)),
    ("v520-ties", (7,)),
    ("v4104-ties", (0, 1, 2, 5, 6, 7)),
    ("v4104-fast", (0, 1, 2, 3, 4, 5)),
    ("v4104-fast", (6,)),
    ("v4104-fast-greedy", (0, 1, 2, 3, 4, 5)),
    ("v128256-fast", (0, 1, 2, 3, 4, 5)),
    ("v128256-fast", (1,)),
    ("v520-cold", (0, 1, 2, 3, 4, 5)),
    # one logits row; the rows differ only in top_k, or only in top_p
    ("v520-topk-capped", (0, 1, 2, 3, 4, 5)),
    ("v520-topp-capped", (0, 1, 2, 3, 4, 5)),
    ("v520-topp-capped", (2, 3, 4, 5, 6, 7)),
)


@pytest.fixture(scope="module")
def tail_engine():
    mp = pytest.MonkeyPatch()
    mp.setenv("OLLAMAMQ_GRAPH_TOPK", "1")
    try:
        eng = _engine("tiny")
    finally:
        mp.undo()
    assert eng._GRAPH_TOPK
    return eng


@pytest.mark.parametrize("name,rows", TAIL_CASES,
                         ids=[f"{n}-B{len(r)}-r{r[0]}" for n, r in TAIL_CASES])
def test_class2_tail_eager(name, rows, tail_engine, monkeypatch):
    hip = _hip()
    eng = tail_engine
    c = so.case(name)
    B, V = len(rows), c["logits"].shape[1]
    C = min(256, V)
    bud, gamma_p, _, _ = so.budget(name)
    logits = c["logits"][list(rows)].to(DEV)
    T = [c["T"][r] for r in rows]
    K = [c["top_k"][r] for r in rows]
    P = [c["top_p"][r] for r in rows]
    assert all(so._f32(t) <= 0 or 0 < k <= 256 for t, k in zip(T, K))
    eng._graphs.pop((B, 2), None)
    entry = eng._graph_entry(B, 2)
    assert entry["graph"] is None
    bufs = entry["bufs"]
    rec = {}
    real = hip.sample_gumbel

    def spy(lg, temps, seeds, ctrs, noise=None, out=None):
        ci = real(lg, temps, seeds, ctrs, noise=noise, out=out)
        rec["vm"], rec["ci"] = lg.float().cpu(), ci.cpu()
        rec["ctrs"] = ctrs
        return ci

    monkeypatch.setattr(hip, "sample_gumbel", spy)
    worst_amb = picks = 0
    tight = np.inf
    for ctr in TAIL_CTRS:
        seeds = [TAIL_SEEDS[(i + ctr) % 4] for i in range(B)]
        bufs["temps"].copy_(torch.tensor(T, dtype=torch.float32))
        bufs["seeds"].copy_(torch.tensor(seeds, dtype=torch.int64))
        bufs["lens"].fill_(ctr)
        bufs["pos"].fill_(7)             # not the counter
        bufs["topk"].copy_(torch.tensor(K, dtype=torch.int64))
        bufs["topp"].copy_(torch.tensor(P, dtype=torch.float32))
        toks = eng._graph_tail(entry, logits).tolist()
        torch.cuda.synchronize()
        assert rec["ctrs"] is bufs["lens"]
        vm, ci = rec["vm"].double().numpy(), rec["ci"].tolist()
        assert vm.shape == (B, C)
        for i, r in enumerate(rows):
            what = f"{name} row {r} ctr {ctr}"
            row = c["logits"][r]
            d = so.filtered_distribution(row, T[i], K[i], P[i])
            if d.greedy:
                assert toks[i] == d.token, \
                    f"{what}: greedy {toks[i]}, lowest-index {d.token}"
                continue
            fin = np.isfinite(vm[i])
            n_seen = int(fin.sum())
            assert fin[:n_seen].all(), f"{what}: kept ranks not a prefix"
            amb = so.boundary_margin(d) < gamma_p
            worst_amb += amb
            want_fin = int(np.isfinite(d.raw[:d.n]).sum())
            if n_seen != want_fin:
                assert amb and abs(n_seen - want_fin) == 1, \
                    f"{what}: {n_seen} candidates kept, oracle {want_fin}"
            assert (vm[i][:n_seen] == d.raw[:n_seen]).all(), \
                f"{what}: kept values are not the oracle's"
            assert so.class2_ok(vm[i], T[i], seeds[i], ctr, ci[i]), \
                f"{what}: candidate {ci[i]}, expected " \
                f"{so.class2_expected(vm[i], T[i], seeds[i], ctr)}"
            assert float(row[toks[i]]) == vm[i][ci[i]], \
                f"{what}: token {toks[i]} is not candidate {ci[i]}"
            picks += 1
            tight = min(tight, so.class2_expected(
                vm[i], T[i], seeds[i], ctr)[2] / so.class2_gamma(vm[i], T[i]))
    assert worst_amb == 0
    # the scaled margin of class2_gamma never decided a pick: every one
    # was compared exactly
    assert tight >= 1, tight
    print(f"RATIO class2-tail {name} B={B}: {picks} picks, kept values "
          f"exact, smallest gap / gamma {tight:.3g}")
    eng._graphs.pop((B, 2), None)


def test_samp_class_rule(tail_engine):
    """Class 2 only when every stochastic row has 0 < top_k <= 256."""
    from ollamamq_amd.engine import GenParams

    class S:
        def __init__(self, **kw):
            self.params = GenParams(**kw)

    eng = tail_engine
    g, t = S(), S(temperature=0.7)
    k5 = S(temperature=0.7, top_k=5)
    k256 = S(temperature=1.0, top_k=256, top_p=0.9)
    k257 = S(temperature=1.0, top_k=257)
    ponly = S(temperature=1.0, top_p=0.5)
    assert eng._samp_class([g]) == 0 and eng._samp_class([g, t]) == 1
    assert eng._samp_class([g, k5, k256]) == 2
    assert eng._samp_class([k5, k257]) == 3
    assert eng._samp_class([k5, ponly]) == 3
    assert eng._samp_class([k5, t]) == 3
    assert eng._samp_class([S(temperature=0.0, top_k=900), k5]) == 2
    eng._GRAPH_TOPK = False
    try:
        assert eng._samp_class([g, k5]) == 3
    finally:
        eng._GRAPH_TOPK = True


# ---------------------------------------------------------------------------
# engine, class 3 (the default host path)


def test_engine_host_sampling_in_support():
    from ollamamq_amd.engine import GenParams
    name = "tiny"
    eng = _engine(name, seed=5)
    tap = Tap(eng)
    import model_oracle as mo
    prompts = mo.case_tokens(name, "host-sampled", (14, 9, 21, 11, 17))
    n = 22
    params = [
        GenParams(max_tokens=n, temperature=0.8, top_k=5, seed=2 ** 63 + 11),
        GenParams(max_tokens=n, temperature=1.0, top_k=40, top_p=0.9),
        GenParams(max_tokens=n, temperature=1.3, top_p=0.5, seed=7),
        GenParams(max_tokens=n, temperature=0.7),
        GenParams(max_tokens=n)]
    seqs = _submit(eng, prompts, params)
    assert seqs[0].noise_seed == 2 ** 63 + 11 - 2 ** 64
    _drive(eng)
    assert all(k[1] == 0 for k in eng._graphs), eng._graphs.keys()
    rows = {(sid, p): row for sid, p, row in tap.events}
    for s in seqs:
        p = s.params
        assert len(s.generated) == n
        for k, t in enumerate(s.generated):
            row = rows[(s.seq_id, len(s.prompt) + k - 1)].cpu()
            assert so.in_support(row, t, p.temperature, p.top_k or 0,
                                 p.top_p or 1.0), \
                f"seq {s.seq_id} token {k} = {t} outside the support"
    _check(name, tap, seqs, "host class-3", tail="host")
