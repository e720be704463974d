"""Logit penalties on the GPU: the HIP kernel (k_logit_penalty through
ops.hip.penalize_logits) against the fp64 oracle of tests/pen_oracle.py at
the shared cases, under graph capture, and inside the engine's eager,
graphed and pipelined decode paths on `tiny`.

Budget of the real tier: 2^-7 |truth| + 2^-8 rms(row), of which one
correct bf16 rounding uses half (fused_oracle.assert_bf16_close).  The
worst ratios are printed as RATIO lines; docs/KERNELS.md records them
(MI355X: 0.422 at V64-B6-real, no bf16 value apart from the fp32 CPU
reference's)."""
import functools

import numpy as np
import pytest
import torch

import elem_oracle as eo
import model_oracle as mo
import pen_oracle as po

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = po.cases()
IDS = [po.case_id(k) for k in CASES]


# ---------------------------------------------------------------------------
# kernel


@functools.lru_cache(maxsize=None)
def scratch(V):
    """One count scratch per vocabulary, zeroed once and shared by every
    call of this file: the kernel must leave it all zero."""
    return torch.zeros((max(po.BS), V), dtype=torch.int32, device=DEV)


def _gpu(c):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v)
            for k, v in c.items()}


def _call(g, counts):
    from ollamamq_amd.ops import hip
    hip.require()
    logits, hist = g["logits"].clone(), g["hist"].clone()
    out = hip.penalize_logits(logits, hist, *(g[a] for a in po.ARGS[2:]),
                              counts)
    torch.cuda.synchronize()
    assert out is logits
    return logits, hist


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_kernel_matches_oracle(key):
    from ollamamq_amd.ops import reference as ref
    c = po.make_case(*key)
    g = _gpu(c)
    counts = scratch(key[0])
    worst = 0.0
    for rep in range(2):     # the second call reuses the scratch as left
        logits, hist = _call(g, counts)
        assert not bool(counts.any()), f"counts not zero after call {rep}"
        worst = max(worst, po.check_against_oracle(
            key, logits, hist, f"kernel call {rep}"))
    # the inputs the kernel only reads are unchanged
    for a in po.ARGS[2:]:
        assert torch.equal(g[a].cpu(), c[a]), a
    # figure, not a requirement: the fp32 host reference rounds each step
    # the same way, so the two usually agree bit for bit
    rl, rh = c["logits"].clone(), c["hist"].clone()
    ref.penalize_logits(rl, rh, *(c[a] for a in po.ARGS[2:]))
    diff = int((rl.view(torch.int16) != logits.cpu().view(torch.int16)).sum())
    print(f"RATIO penalty-kernel {po.case_id(key)} {worst:.3f} "
          f"bits-differing-from-reference {diff}")


def test_wrapper_rejects_bad_arguments():
    from ollamamq_amd.ops import hip
    hip.require()
    g = _gpu(po.make_case(520, 6, "exact"))
    counts = scratch(520)
    args = [g[a] for a in po.ARGS]

    def call(**kw):
        a = dict(zip(po.ARGS, (t.clone() for t in args)), counts=counts)
        a.update(kw)
        return hip.penalize_logits(*(a[k] for k in po.ARGS), a["counts"])

    call()
    with pytest.raises(ValueError):
        call(logits=g["logits"].float())
    with pytest.raises(ValueError):
        call(logits=g["logits"].t().contiguous().t())
    with pytest.raises(ValueError):
        call(logits=torch.zeros((6, 1040), dtype=torch.bfloat16,
                                device=DEV)[:, ::2])
    with pytest.raises(ValueError):
        call(counts=torch.zeros((6, 519), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        call(counts=torch.zeros((5, 520), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        call(hist=g["hist"].long())
    with pytest.raises(ValueError):
        call(rp=g["rp"].double())
    with pytest.raises(ValueError):
        call(lens=g["lens"].long())
    torch.cuda.synchronize()
    assert not bool(counts.any())


def test_kernel_under_graph_capture():
    """The op captured with tok / lens advanced on-device by a trailing
    add and replayed three times equals three eager steps bit for bit,
    hist included: the captured kernel reads lens and tok from memory at
    replay, appends, and leaves the scratch zero for the next replay."""
    from ollamamq_amd.ops import hip
    hip.require()
    V, B, steps = 520, 6, 3
    g = torch.Generator().manual_seed(77)
    hist0 = torch.randint(0, V, (po.MAX_SLOTS, po.MAX_CTX), generator=g).int()
    slot = torch.tensor([9, 3, 60, 0, 41, 17], dtype=torch.int32)
    lens0 = torch.tensor([1, 14, 62, 63, 100, 253], dtype=torch.int32)
    tok0 = torch.tensor([5, 0, 516, 7, -1, 100], dtype=torch.int32)
    # a row without append stays one: its tok is held by an advance of 0
    adv_tok = (tok0 >= 0).int()
    last_n = torch.tensor([-1, 4, 64, 0, 65, 10 ** 6], dtype=torch.int32)
    rp = torch.tensor([1.1, 1.3, 0.8, 2.0, 1.0, 1.3])
    pp = torch.tensor([0.5, 0.0, -0.7, 1.0, 0.0, 1.9])
    fp = torch.tensor([0.0, 0.5, 1.9, 1.0, 0.0, -0.7])
    fresh = [(torch.randn((B, V), generator=g) * 2).bfloat16()
             for _ in range(steps)]
    # the oracle follows the three steps on the CPU
    want, h, lens, tok = [], hist0.clone(), lens0.clone(), tok0.clone()
    for i in range(steps):
        x, touched, hn = po.oracle(fresh[i], h, slot, lens, tok, last_n,
                                   rp, pp, fp)
        want.append((torch.from_numpy(x), torch.from_numpy(touched)))
        h = torch.from_numpy(hn)
        lens, tok = lens + 1, tok + adv_tok
    d = lambda t: t.to(DEV)                                   # noqa: E731
    slot_d, last_d, rp_d, pp_d, fp_d, adv_d = map(
        d, (slot, last_n, rp, pp, fp, adv_tok))
    counts = scratch(V)
    hist, lens_d, tok_d = d(hist0), d(lens0), d(tok0)
    lg = torch.empty((B, V), dtype=torch.bfloat16, device=DEV)

    def step():
        hip.penalize_logits(lg, hist, slot_d, lens_d, tok_d, last_d,
                            rp_d, pp_d, fp_d, counts)
        tok_d.add_(adv_d)
        lens_d.add_(1)

    # eager: also the warm-up of the capture, on a side stream
    eager = []
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for i in range(steps):
            lg.copy_(d(fresh[i]))
            step()
            eager.append(lg.clone())
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager_hist = hist.clone()
    assert torch.equal(eager_hist.cpu(), h)
    for i, (x, touched) in enumerate(want):
        got = eager[i].cpu()
        assert torch.equal(got[~touched], fresh[i][~touched])
        err = (got.double() - x).abs()
        rms = x.pow(2).mean(-1, keepdim=True).sqrt()
        assert bool((err <= x.abs() * 2.0 ** -7 + rms * 2.0 ** -8).all()), i
    # reset, capture, replay
    hist.copy_(d(hist0))
    lens_d.copy_(d(lens0))
    tok_d.copy_(d(tok0))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    # capture runs nothing
    assert torch.equal(lens_d.cpu(), lens0)
    for i in range(steps):
        lg.copy_(d(fresh[i]))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(lg, eager[i]), f"replay {i} differs from eager"
        assert not bool(counts.any())
    assert torch.equal(hist, eager_hist)
    assert torch.equal(lens_d.cpu(), lens0 + steps)


# ---------------------------------------------------------------------------
# engine on `tiny`

NAME = "tiny"
PATHS = ("eager", "graphed", "pipelined")


@functools.lru_cache(maxsize=None)
def gpu_model():
    from ollamamq_amd.models import LlamaModel
    return LlamaModel(mo.config(NAME), device=DEV, dtype=torch.bfloat16,
                      seed=mo.SEED)


def _engine(seed=0):
    from ollamamq_amd.engine import LlamaEngine, PagedKVCache
    model = gpu_model()
    kv = PagedKVCache.for_model(model.cfg, n_pages=96, max_slots=10,
                                max_ctx=mo.MAX_CTX, device=DEV,
                                dtype=torch.bfloat16)
    mo.scramble(kv, seed)
    return LlamaEngine(model, kv, max_batch=8)


def _set_path(eng, path):
    eng.use_graphs = path != "eager"
    eng.use_pipeline = path == "pipelined"


def _run(eng, prompts, params):
    """Drive to the end.  With a penalty in the batch, also: the device
    history of every sequence holds its tokens, each at its own position
    (all but the last, which is never fed back), and on the graphed paths
    the host applies the penalty to rows finishing a prefill only: a
    penalised entry's logits come penalised out of the graph."""
    seqs = [eng.seqs[eng.submit(list(p), g)] for p, g in zip(prompts, params)]
    host_calls = []
    orig = eng._penalize

    def spy(sq, logits, pen_tok):
        host_calls.append(list(pen_tok))
        return orig(sq, logits, pen_tok)

    eng._penalize = spy
    slots = {}
    try:
        for _ in range(400):
            eng.step()
            for s in seqs:
                if s.slot >= 0:
                    slots[s.seq_id] = s.slot
            if not eng.has_work():
                break
    finally:
        eng._penalize = orig
    assert not eng.has_work(), "engine did not drain"
    torch.cuda.synchronize()
    if any(g.penalty_active for g in params):
        hist = eng._hist.cpu()
        # the rows are read after the run: no slot may have served two of
        # the sequences, or one would be read where another wrote last
        assert len(set(slots.values())) == len(seqs), \
            f"a slot was reused within the run: {slots}"
        for s in seqs:
            full = s.prompt + s.generated
            if s.params.penalty_active or len(s.generated) > 1:
                n0 = 0 if s.params.penalty_active else len(s.prompt)
                assert hist[slots[s.seq_id], n0:len(full) - 1].tolist() \
                    == full[n0:-1], f"history of sequence {s.seq_id}"
        if eng.use_graphs:
            assert host_calls and all(
                t == -1 for call in host_calls for t in call), host_calls
    return seqs


def _gp(n, **kw):
    from ollamamq_amd.engine import GenParams
    return GenParams(max_tokens=n, **kw)


PROMPT_LENS = (10, 58, 60, 30, 12)
MAX_TOKENS = (40, 40, 40, 20, 20)


def _mixed_params():
    """Penalised and unpenalised rows in one batch of five (bucket 6, one
    pad row); two finish after 20 tokens, the rest go on in bucket 3.  The
    10- and 58-token prompts cross lengths 15 -> 16 and 63 -> 64."""
    kws = (dict(repeat_penalty=1.3, presence_penalty=0.5,
                frequency_penalty=0.25),
           dict(),
           dict(presence_penalty=1000.0, repeat_last_n=-1),
           dict(repeat_penalty=1.1, repeat_last_n=4, frequency_penalty=1.9),
           dict(repeat_penalty=5.0, repeat_last_n=0))
    return [_gp(n, **kw) for n, kw in zip(MAX_TOKENS, kws)]


def _window_tokens(full, at, n):
    w = at if (n < 0 or n > at) else n
    return full[at - w:at]


def _pen_row(L, full, at, p):
    """fp64 penalised logits of one position: the oracle applied to the
    model oracle's row L over the sequence's first `at` tokens."""
    hist = torch.zeros((1, mo.MAX_CTX), dtype=torch.int32)
    hist[0, :at] = torch.tensor(full[:at], dtype=torch.int32)
    i32 = lambda v: torch.tensor([v], dtype=torch.int32)       # noqa: E731
    f32 = lambda v: torch.tensor([v], dtype=torch.float32)     # noqa: E731
    x, _, _ = po.oracle(L.reshape(1, -1), hist, i32(0), i32(at), i32(-1),
                        i32(p.repeat_last_n), f32(p.repeat_penalty),
                        f32(p.presence_penalty), f32(p.frequency_penalty))
    return x[0]


def _check_trajectory(seqs, what):
    """Teacher forcing: every produced token against the fp64 model oracle
    with the penalty oracle on top.  gamma = 2 x budget.logits_mx x rms(L),
    as model_oracle.greedy_ok; a repeat penalty below 1 stretches logit
    errors by 1 / rp, hence the factor max(1, 1 / rp)."""
    full = [s.prompt + s.generated for s in seqs]
    truth, budget = mo.truth_and_budget(mo.cpu_model(NAME), full)
    worst = float("inf")
    for i, s in enumerate(seqs):
        p = s.params
        stretch = max(1.0, 1.0 / p.repeat_penalty)
        for k, t in enumerate(s.generated):
            at = len(s.prompt) + k
            L = truth.logits[i][at - 1].double()
            gamma = 2.0 * budget.logits_mx * float(L.pow(2).mean().sqrt())
            P = _pen_row(L, full[i], at, p)
            if p.temperature <= 0:
                slack = P[t] - (P.max() - gamma * stretch)
                assert slack >= 0, \
                    f"{what}: seq {i} token {k} is not near the penalised best"
                worst = min(worst, float(slack))
            elif k > 0:
                # in-graph Gumbel tail, counter = the KV length = at
                T = p.temperature
                u = eo.hash_u01(s.noise_seed, at,
                                np.arange(P.shape[0], dtype=np.int64))
                sc = P / T - np.log(-np.log(u.astype(np.float64)))
                tol = gamma * stretch / T + eo.GUMBEL_GAMMA
                assert sc[t] >= sc.max() - tol, \
                    f"{what}: seq {i} token {k} is not the penalised Gumbel pick"
    return worst


def _assert_distinct(seq):
    assert len(seq.prompt) + len(seq.generated) < mo.config(NAME).vocab
    assert len(set(seq.generated)) == len(seq.generated), seq.generated
    assert not set(seq.generated) & set(seq.prompt), seq.generated


def _assert_window_distinct(seq, n):
    all_t = seq.prompt + seq.generated
    for i in range(len(seq.prompt), len(all_t)):
        assert all_t[i] not in all_t[max(0, i - n):i], (i, all_t)


def test_engine_three_paths_mixed_batch():
    eng = _engine()
    prompts = mo.case_tokens(NAME, "penalty", PROMPT_LENS)
    runs = {}
    for path in PATHS:
        _set_path(eng, path)
        seqs = _run(eng, prompts, _mixed_params())
        for s, n in zip(seqs, MAX_TOKENS):
            assert len(s.generated) == n
        runs[path] = seqs
    for path in PATHS[1:]:
        for a, b in zip(runs["eager"], runs[path]):
            assert a.generated == b.generated, \
                f"{path} differs from eager: {a.generated} vs {b.generated}"
    assert set(eng._graphs) == {(6, 0, 1), (3, 0, 1)}
    # the pad row of bucket 6: switched off, on the dummy slot, never
    # advanced, and the unpenalised rows switched off too
    bufs = eng._graphs[(6, 0, 1)]["bufs"]
    assert bufs["last_n"].tolist() == [64, 0, -1, 4, 0, 0]
    assert bufs["slot"][5].item() == eng._dummy_slot
    assert bufs["adv"].tolist() == [1] * 5 + [0]
    assert bufs["lens"][5].item() == 1
    assert not bool(eng._counts.any())
    _assert_distinct(runs["eager"][2])
    # the penalties did something, and the unpenalised neighbours are the
    # tokens of a run without any penalty in the batch
    plain = _engine()
    _set_path(plain, "pipelined")
    base = _run(plain, prompts, [_gp(n) for n in MAX_TOKENS])
    assert all(len(k) == 2 for k in plain._graphs) and plain._graphs
    assert plain._hist is None and plain._counts is None
    assert base[0].generated != runs["eager"][0].generated
    slack = _check_trajectory(runs["pipelined"], "pipelined mixed batch")
    _check_trajectory(base, "unpenalised")
    print(f"RATIO penalty-engine least greedy slack {slack:.4f}")


def test_engine_sampled_row_through_gumbel_tail():
    """Class 1: a penalised temperature row and a penalised greedy row in
    the in-graph Gumbel tail."""
    eng = _engine(seed=1)
    prompts = mo.case_tokens(NAME, "penalty-sampled", (14, 9))
    params = [_gp(24, temperature=0.8, seed=11, repeat_penalty=1.3,
                  presence_penalty=0.5),
              _gp(24, repeat_penalty=0.8, frequency_penalty=0.5,
                  repeat_last_n=-1)]
    seqs = _run(eng, prompts, params)
    assert set(eng._graphs) == {(2, 1, 1)}
    _check_trajectory(seqs, "class-1 penalised")


def test_engine_distinctness_on_every_path():
    """presence_penalty = 1000: no token repeats inside the window, on the
    first token after the prefill too, with a class-3 row (top_p = 0.5,
    sampled on the host from the penalised entry's logits) in the batch."""
    prompts = mo.case_tokens(NAME, "penalty-distinct", (20, 9, 33))
    for path in PATHS:
        eng = _engine(seed=2)
        _set_path(eng, path)
        # a window past the int32 range is the whole sequence
        params = [_gp(30, presence_penalty=1000.0,
                      repeat_last_n=3000000000),
                  _gp(30, presence_penalty=1000.0, repeat_last_n=-1,
                      temperature=0.8, top_p=0.5, seed=3),
                  _gp(30, presence_penalty=1000.0, repeat_last_n=4)]
        seqs = _run(eng, prompts, params)
        assert [len(s.generated) for s in seqs] == [30, 30, 30]
        _assert_distinct(seqs[0])
        _assert_distinct(seqs[1])
        _assert_window_distinct(seqs[2], 4)
        if path != "eager":
            # class 3 decodes on the class-0 graph and samples on the host
            assert set(eng._graphs) == {(3, 0, 1)}, set(eng._graphs)


def test_warm_graphs_penalty_flag():
    eng = _engine(seed=3)
    eng.warm_graphs(sizes=(1, 2), classes=(0,))
    assert set(eng._graphs) == {(1, 0), (2, 0)} and eng._hist is None
    eng.warm_graphs(sizes=(1, 2), classes=(0,), penalty=True)
    assert set(eng._graphs) == {(1, 0), (2, 0), (1, 0, 1), (2, 0, 1)}
    assert all(e["graph"] is not None for e in eng._graphs.values())
    assert not bool(eng._counts.any())
    assert len(eng.kv._free_slots) == eng.kv.max_slots
    seqs = _run(eng, mo.case_tokens(NAME, "penalty-warm", (7,)),
                [_gp(20, presence_penalty=1000.0, repeat_last_n=-1)])
    _assert_distinct(seqs[0])
