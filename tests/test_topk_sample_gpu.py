"""ops.hip.sample_topk (topk_sample.hip): the exact top-256 selection against
a stable fp64 argsort, the filter and the pick against the fp64 distribution
oracle (tests/sampler_oracle.py) with the margins of the class-2 tail's own
test, bit-equality of eager calls and graph replays, and the engine's class-2
tail under OLLAMAMQ_GRAPH_TOPK=hip."""
import numpy as np
import pytest
import torch

import sampler_oracle as so
from test_engine_oracle_gpu import Tap, _drive, _engine, _submit

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEEDS = (0, -1, 2 ** 63 - 1, -2 ** 63)
CTRS = (1, 4095)
# tests/test_sampler_paths_gpu.py TAIL_CASES: every stochastic row has
# 0 < top_k <= 256
R6 = (0, 1, 2, 3, 4, 5)
TAIL_CASES = (
    ("v520-ties", R6), ("v520-ties", (6,)), ("v520-ties", (7,)),
    ("v4104-ties", (0, 1, 2, 5, 6, 7)), ("v4104-fast", R6),
    ("v4104-fast", (6,)), ("v4104-fast-greedy", R6), ("v128256-fast", R6),
    ("v128256-fast", (1,)), ("v520-cold", R6), ("v520-topk-capped", R6),
    ("v520-topp-capped", R6), ("v520-topp-capped", (2, 3, 4, 5, 6, 7)),
)


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


def _run(hip, logits, T, K, P, seeds, ctr):
    """One call with the candidate triple; everything back on the host."""
    B = logits.shape[0]
    t = lambda x, dt: torch.tensor(x, dtype=dt, device=DEV)
    cand = (torch.full((B, 256), 7.0, device=DEV),
            torch.full((B, 256), -7, dtype=torch.int32, device=DEV),
            torch.full((B,), -7, dtype=torch.int32, device=DEV))
    toks = hip.sample_topk(
        logits.to(DEV), t(T, torch.float32), t(K, torch.int64),
        t(P, torch.float32), t(seeds, torch.int64),
        t([ctr] * B, torch.int32), cand=cand)
    torch.cuda.synchronize()
    return (toks.tolist(), cand[0].double().cpu().numpy(),
            cand[1].cpu().numpy(), cand[2].tolist())


def _hand(name):
    """Hand-made rows, [n, V] fp32 (every value a bf16)."""
    g = torch.Generator().manual_seed(len(name))
    if name == "flat-520":
        return torch.full((1, 520), 0.5)
    if name == "zeros-520":         # +0.0 / -0.0 mixed, three positives
        x = torch.zeros(1, 520)
        x[0, 1::2] = -0.0
        x[0, [7, 300, 519]] = torch.tensor([1.0, 2.0, 1.0])
        return x
    if name in ("v263", "v4101"):   # V % 8 != 0: above C, behind full slices
        return torch.randn(2, int(name[1:]), generator=g) * 2.0
    if name == "v128256-last-slice":
        # 250 values above the threshold, all in the last slice; 300 copies
        # of the threshold, 8.0, over every slice: the 6 lowest ids are in
        V = 128256
        x = (torch.randn(1, V, generator=g) * 2.0).clamp(max=6.0)
        x[0, V - 250:] = 16.0 + torch.arange(250) % 50
        x[0, torch.linspace(0, V - 251, 300).long()] = 8.0
        return x
    x = torch.randn(1, 520, generator=g) * 2.0
    if name == "one-finite-520":
        x[:] = float("-inf")
        x[0, 173] = 1.25
    else:                           # "inf-block-520"
        x[0, 100:400] = float("-inf")
    return x


SHARED = ("v64-mixed", "v520-ties", "v4104-ties", "v128256-fast")
HAND = ("flat-520", "zeros-520", "v263", "v4101", "v128256-last-slice",
        "one-finite-520", "inf-block-520")


@pytest.mark.parametrize("name", SHARED + HAND)
def test_candidates_exact(name):
    if name in SHARED:
        c = so.case(name)
        logits, T = c["logits"], c["T"]
    else:                           # every hand-made row greedy and sampled
        logits = _hand(name).bfloat16().repeat_interleave(2, 0)
        T = [0.0, 1.0] * (logits.shape[0] // 2)
    B, V = logits.shape
    C = min(256, V)
    _, _, ids, _ = _run(_hip(), logits, T, [40] * B, [0.9] * B, [3] * B, 9)
    for b in range(B):
        want = np.argsort(-logits[b].double().numpy(), kind="stable")[:C]
        assert (ids[b, :C] == want).all(), \
            f"{name} row {b}: first miss at rank " \
            f"{int(np.flatnonzero(ids[b, :C] != want)[0])}"
        assert (ids[b, C:] == -7).all(), "columns >= C were written"


@pytest.mark.parametrize("name,rows", TAIL_CASES,
                         ids=[f"{n}-B{len(r)}-r{r[0]}" for n, r in TAIL_CASES])
def test_filter_and_pick(name, rows):
    hip = _hip()
    c = so.case(name)
    B = len(rows)
    _, gamma_p, _, _ = so.budget(name)
    T = [c["T"][r] for r in rows]
    K = [c["top_k"][r] for r in rows]
    P = [c["top_p"][r] for r in rows]
    n_amb = picks = 0
    tight = np.inf
    for ctr in CTRS:
        seeds = [SEEDS[(i + ctr) % 4] for i in range(B)]
        toks, vals, ids, pick = _run(hip, c["logits"][list(rows)], T, K, P,
                                     seeds, ctr)
        for i, r in enumerate(rows):
            what = f"{name} row {r} ctr {ctr}"
            row = c["logits"][r]
            d = so.filtered_distribution(row, T[i], K[i], P[i])
            if d.greedy:
                assert toks[i] == d.token and pick[i] == 0, what
                continue
            vm = vals[i][:min(256, d.V)]
            fin = np.isfinite(vm)
            n_seen = int(fin.sum())
            assert fin[:n_seen].all(), f"{what}: kept ranks not a prefix"
            amb = so.boundary_margin(d) < gamma_p
            n_amb += amb
            want_fin = int(np.isfinite(d.raw[:d.n]).sum())
            if n_seen != want_fin:
                assert amb and abs(n_seen - want_fin) == 1, \
                    f"{what}: {n_seen} candidates kept, oracle {want_fin}"
            assert (vm[:n_seen] == d.raw[:n_seen]).all(), \
                f"{what}: kept values are not the oracle's"
            assert so.class2_ok(vm, T[i], seeds[i], ctr, pick[i]), \
                f"{what}: rank {pick[i]}, expected " \
                f"{so.class2_expected(vm, T[i], seeds[i], ctr)}"
            assert float(row[toks[i]]) == vm[pick[i]] \
                and toks[i] == ids[i][pick[i]], what
            picks += 1
            tight = min(tight, so.class2_expected(
                vm, T[i], seeds[i], ctr)[2] / so.class2_gamma(vm, T[i]))
    n_stoch = sum(so._f32(t) > 0 for t in T) * len(CTRS)
    assert n_amb <= so.AMBIGUOUS_CAP * n_stoch, (name, n_amb)
    print(f"RATIO topk-sample {name} B={B}: {picks} picks, smallest gap / "
          f"gamma {tight:.3g}, {n_amb} ambiguous rows")


def test_deterministic_under_graph():
    hip = _hip()
    c = so.case("v4104-fast")
    B = 6
    t = lambda x, dt: torch.tensor(x[:B], dtype=dt, device=DEV)
    logits = c["logits"][:B].to(DEV)
    args = (logits, t(c["T"], torch.float32), t(c["top_k"], torch.int64),
            t(c["top_p"], torch.float32), t(list(range(B)), torch.int64))
    ctrs = torch.full((B,), 5, dtype=torch.int32, device=DEV)
    out = torch.empty(B, dtype=torch.int32, device=DEV)
    cand = (torch.zeros((B, 256), device=DEV),
            torch.zeros((B, 256), dtype=torch.int32, device=DEV),
            torch.zeros(B, dtype=torch.int32, device=DEV))

    def step():
        hip.sample_topk(*args, ctrs, out=out, cand=cand)
        ctrs.add_(1)

    eager = []
    for _ in range(3):
        step()
        eager.append([x.clone() for x in (out, *cand)])
    assert not torch.equal(eager[0][0], eager[2][0]) \
        or not torch.equal(eager[0][3], eager[2][3])   # the counter matters
    ctrs.fill_(5)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for k in range(3):
        g.replay()
        for got, want in zip((out, *cand), eager[k]):
            assert torch.equal(got, want), f"replay {k} differs from eager"
    for bad in ((logits.float(), *args[1:], ctrs),
                (logits[:, ::2], *args[1:], ctrs),
                (logits[0], *args[1:], ctrs),
                (logits, args[1][:B - 1], *args[2:], ctrs),
                (logits, args[1], args[2].int(), *args[3:], ctrs),
                (*args, ctrs.long()),
                (*args[:4], args[4].cpu(), ctrs)):
        with pytest.raises(ValueError):
            hip.sample_topk(*bad)
    with pytest.raises(ValueError):
        hip.sample_topk(*args, ctrs, cand=(cand[0][:, :128], *cand[1:]))


def test_engine_hip_tail(monkeypatch):
    from ollamamq_amd.engine import GenParams
    hip = _hip()
    monkeypatch.setenv("OLLAMAMQ_GRAPH_TOPK", "hip")
    # the in-graph tail runs on the pipelined path only: the non-pipelined
    # decode replays a class-0 graph and samples on the host
    eng = _engine("tiny", seed=6)
    assert eng._GRAPH_TOPK and eng._TOPK_HIP and eng.use_pipeline

    def no_torch_tail(*a, **k):
        raise AssertionError("candidate_filter ran under the hip tail")

    tap = Tap(eng)
    n = 14
    params = [GenParams(max_tokens=n, temperature=0.8, top_k=1),
              GenParams(max_tokens=n, temperature=0.9, top_k=5, top_p=0.9,
                        seed=42),
              GenParams(max_tokens=n)]
    prompt = [2, 7, 1, 8, 2, 8]
    seqs = _submit(eng, [prompt] * 3, params)
    while not all(s.state == "running" for s in seqs):
        eng.step()                  # first tokens: sampled on the host
    monkeypatch.setattr(hip, "candidate_filter", no_torch_tail)
    _drive(eng)
    monkeypatch.undo()
    assert all(len(s.generated) == n for s in seqs)
    assert any(k[1] == 2 for k in eng._graphs), eng._graphs.keys()
    rows = {(sid, p): row for sid, p, row in tap.events}
    greedy = _submit(eng, [prompt], [GenParams(max_tokens=n)])[0]
    _drive(eng)
    assert seqs[0].generated == greedy.generated, "top_k = 1 is not greedy"
    assert seqs[2].generated == greedy.generated, "the greedy row drifted"
    s1 = seqs[1]
    t = lambda x, dt: torch.tensor([x], dtype=dt, device=DEV)
    for k, tok in enumerate(s1.generated):
        at = len(s1.prompt) + k
        row = rows[(s1.seq_id, at - 1)]
        assert so.in_support(row.cpu(), tok, 0.9, 5, 0.9), \
            f"token {k} = {tok} outside its step's support"
        if k:                       # the first token is sampled on the host
            want = hip.sample_topk(
                row.unsqueeze(0).contiguous(), t(0.9, torch.float32),
                t(5, torch.int64), t(0.9, torch.float32),
                t(s1.noise_seed, torch.int64), t(at, torch.int32))
            assert tok == int(want[0]), f"token {k}: graph {tok}, eager " \
                                        f"{int(want[0])}"
