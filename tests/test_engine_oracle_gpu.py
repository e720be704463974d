"""LlamaEngine's decode step held to the fp64 model oracle by teacher
forcing (tests/model_oracle.py): after a run the oracle is evaluated on the
tokens each sequence actually consumed and produced, so every logits row
the engine computed and every token it emitted is checked against truth at
identical inputs, whatever near-ties flipped on the way.

A Tap records each logits row at its source (the generic forward, or the
static buffer of a replayed graph) together with the position the HOST
expects it to belong to, derived from the sequences' own state and never
from the position lists the engine builds: a frozen in-graph position, a
stale length, a dropped window or a chunk numbered from 0 computes the row
of another position and misses the budget."""
import functools

import pytest
import torch

import model_oracle as mo
import sampler_oracle as so

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ENGINE_CONFIGS = ("tiny", "tiny-qwen", "tiny-swa", "qwen-mini")


@functools.lru_cache(maxsize=None)
def gpu_model(name):
    from ollamamq_amd.models import LlamaModel
    m = LlamaModel(mo.config(name), device=DEV, dtype=torch.bfloat16,
                   seed=mo.SEED)
    assert m.fused_chain, f"{name} should qualify for the fused chain"
    return m


def _engine(name, prefill_chunk=2048, seed=0):
    from ollamamq_amd.engine import LlamaEngine, PagedKVCache
    model = gpu_model(name)
    kv = PagedKVCache.for_model(model.cfg, n_pages=96, max_slots=10,
                                max_ctx=mo.MAX_CTX, device=DEV,
                                dtype=torch.bfloat16)
    mo.scramble(kv, seed)
    return LlamaEngine(model, kv, max_batch=8, prefill_chunk=prefill_chunk)


class Tap:
    """Records (seq id, expected position, logits row) for every logits
    row the engine computes for a sequence."""

    def __init__(self, eng):
        self.events, self.modes = [], []
        self.fills = self.replays = 0
        self._filled = {}
        fwd, fill, replay = eng._forward, eng._fill_bufs, eng._graph_replay

        def _forward(seqs, token_list, pos_list, q_lens, mode, n_decode=0):
            exp = [s.total_len - 1 if s.state == "running"
                   else s.prefill_done + ql - 1
                   for s, ql in zip(seqs, q_lens)]
            logits = fwd(seqs, token_list, pos_list, q_lens, mode,
                         n_decode=n_decode)
            self.modes.append((mode, [s.prefill_done for s in seqs
                                      if s.state != "running"]))
            self._note(seqs, exp, logits)
            return logits

        def _fill_bufs(entry, seqs, token_list, pos_list):
            # host truth is current here (the pipe is drained before a fill)
            self._filled[id(entry)] = [list(seqs),
                                       [s.total_len - 1 for s in seqs], 0]
            self.fills += 1
            return fill(entry, seqs, token_list, pos_list)

        def _graph_replay(entry):
            out = replay(entry)
            seqs, pos, k = f = self._filled[id(entry)]
            # the k-th replay after a fill serves the k-th next position
            self._note(seqs, [p + k for p in pos],
                       entry["logits"][:len(seqs)].clone())
            f[2] += 1
            self.replays += 1
            return out

        eng._forward, eng._fill_bufs = _forward, _fill_bufs
        eng._graph_replay = _graph_replay

    def _note(self, seqs, exp, logits):
        assert logits.shape[0] == len(seqs)
        for s, p, row in zip(seqs, exp, logits):
            self.events.append((s.seq_id, p, row))

    def clear(self):
        self.events, self.modes = [], []
        self.fills = self.replays = 0


def _submit(eng, prompts, params):
    return [eng.seqs[eng.submit(list(p), g)] for p, g in zip(prompts, params)]


def _drive(eng, steps=400):
    for _ in range(steps):
        eng.step()
        if not eng.has_work():
            break
    assert not eng.has_work(), "engine did not drain"
    torch.cuda.synchronize()


def _check(name, tap, seqs, what, tail="gumbel"):
    """Teacher-forced check of a finished run.  tail: what samples the
    decode tokens of a stochastic sequence, the in-graph "gumbel" tail or
    the "host" (whose draws the caller checks).  Returns the oracle's
    truth and budget."""
    full = [s.prompt + s.generated for s in seqs]
    truth, budget = mo.truth_and_budget(mo.cpu_model(name), full)
    index = {s.seq_id: i for i, s in enumerate(seqs)}
    got, want, seen = [], [], {}
    for sid, p, row in tap.events:
        i = index[sid]
        if p >= len(full[i]):
            continue    # pipelined: one replay past the last kept token
        got.append(row)
        want.append(truth.logits[i][p])
        seen[(i, p)] = row
    # every emitted token's logits row was recorded
    for i, s in enumerate(seqs):
        assert len(s.generated) >= 20, (what, len(s.generated))
        for k in range(len(s.generated)):
            assert (i, len(s.prompt) + k - 1) in seen, (what, i, k)
    got = torch.stack(got)
    assert torch.isfinite(got).all(), f"{what}: non-finite logits"
    r = budget.hold("logits", got, torch.stack(want), what)
    # trajectory: every produced token
    for i, s in enumerate(seqs):
        T = s.params.temperature
        for k, t in enumerate(s.generated):
            at = len(s.prompt) + k
            L = truth.logits[i][at - 1]
            if T <= 0:
                assert mo.greedy_ok(L, t, budget.logits_mx), \
                    f"{what}: seq {i} token {k} is not near the oracle's best"
            elif k == 0:
                # sampled on the host from the row recorded at the end of
                # the prefill: exact on that row's values, the token lies
                # in the temperature-only support (a finite logit) and
                # inside the sequence's own filters
                p = s.params
                row = seen[(i, at - 1)].cpu()
                assert so.in_support(row, t, T, 0, 1.0) and so.in_support(
                    row, t, T, p.top_k or 0, p.top_p or 1.0), \
                    f"{what}: seq {i} first token outside the support"
            elif tail == "gumbel":
                # the in-graph Gumbel tail: the counter is bufs["lens"],
                # the KV length the tail sees = tokens in the sequence
                # once the fed token is appended = the produced token's
                # own index `at` in the full sequence
                ok, _ = mo.gumbel_ok(L, t, T, s.noise_seed, at,
                                     budget.logits_mx)
                assert ok, f"{what}: seq {i} token {k} is not the " \
                           f"emulated Gumbel pick"
    print(f"RATIO engine-{what.split()[0]} {name} logits {r:.3f}")
    return truth, budget


def _greedy(n):
    from ollamamq_amd.engine import GenParams
    return GenParams(max_tokens=n)


# ---------------------------------------------------------------------------
# one workload, three paths

PROMPT_LENS = (10, 58, 60, 30, 12)
MAX_TOKENS = (40, 40, 40, 20, 20)


@pytest.mark.parametrize("name", ENGINE_CONFIGS)
def test_workload_three_paths(name):
    """Five sequences decode in bucket 6 (one pad row on the dummy slot);
    two finish after 20 tokens and the other three go on in bucket 3 (the
    bucket list holds 3, so three rows are not padded).
    Prompts of 10 and 58 tokens cross positions 15->16 and 63->64 six
    tokens in: pipelined, that is inside one run of replays with no host
    refill.  On tiny-swa the long ones pass the window of 96."""
    eng = _engine(name)
    tap = Tap(eng)
    prompts = mo.case_tokens(name, "engine", PROMPT_LENS)
    for path in ("eager", "graphed", "pipelined"):
        eng.use_graphs = path != "eager"
        eng.use_pipeline = path == "pipelined"
        tap.clear()
        seqs = _submit(eng, prompts, [_greedy(n) for n in MAX_TOKENS])
        _drive(eng)
        for s, n in zip(seqs, MAX_TOKENS):
            assert len(s.generated) == n
        if path == "eager":
            assert tap.replays == 0
        elif path == "graphed":
            assert tap.fills == tap.replays >= 39
        else:
            # a fill at the start and one per composition change only
            assert tap.replays >= 39 and tap.fills <= 3, tap.fills
        _check(name, tap, seqs, f"{path} workload")
    assert set(eng._graphs) == {(6, 0), (3, 0)}


# ---------------------------------------------------------------------------
# late admission


@pytest.mark.parametrize("name", ("tiny", "qwen-mini"))
def test_late_admission_continued_chunks(name):
    """prefill_chunk = 16: a 50-token prompt submitted while two sequences
    decode is prefilled over four mixed steps, three of them continued
    chunks."""
    eng = _engine(name, prefill_chunk=16, seed=1)
    tap = Tap(eng)
    p = mo.case_tokens(name, "late", (20, 9, 50))
    seqs = _submit(eng, p[:2], [_greedy(36), _greedy(36)])
    while not all(s.state == "running" for s in seqs):
        eng.step()
    for _ in range(4):
        eng.step()
    seqs += _submit(eng, p[2:], [_greedy(24)])
    _drive(eng)
    cont = [st for mode, st in tap.modes if mode == "mixed" and st
            and st[0] > 0]
    assert len(cont) == 3 and [st[0] for st in cont] == [16, 32, 48], \
        tap.modes
    _check(name, tap, seqs, "late admission")


# ---------------------------------------------------------------------------
# sliding window under capture


def test_sliding_window_graphed():
    """tiny-swa, a 90-token prompt and 24 tokens: the window of 96 starts
    to cut inside the graphed, then the graphed and pipelined decode."""
    name = "tiny-swa"
    eng = _engine(name, seed=2)
    tap = Tap(eng)
    prompt = mo.case_tokens(name, "swa", (90,))
    for pipelined in (False, True):
        eng.use_pipeline = pipelined
        tap.clear()
        seqs = _submit(eng, prompt, [_greedy(24)])
        _drive(eng)
        assert tap.replays >= 23
        assert tap.fills == (1 if pipelined else tap.replays)
        _check(name, tap, seqs,
               "swa-pipelined" if pipelined else "swa-graphed")


# ---------------------------------------------------------------------------
# sampled decode, class 1 (in-graph Gumbel tail)


def _params(T, seed=None, n=24):
    from ollamamq_amd.engine import GenParams
    return GenParams(max_tokens=n, temperature=T, seed=seed)


def test_sampled_decode_gumbel_tail():
    """Temperatures 0.7 and 1.3, request seeds and engine-default seeds,
    one greedy row, all submitted together: after each sequence's first
    token (sampled on the host) every token comes from the in-graph tail
    and must be the emulated Gumbel pick."""
    name = "tiny"
    eng = _engine(name, seed=3)
    tap = Tap(eng)
    prompts = mo.case_tokens(name, "sampled", (14, 9, 21, 11, 17))
    params = [_params(0.7, 11), _params(1.3), _params(0.0),
              _params(1.3, 5), _params(0.7)]
    seqs = _submit(eng, prompts, params)
    _drive(eng)
    assert set(eng._graphs) == {(6, 1)} and tap.fills == 1
    _check(name, tap, seqs, "sampled class-1")


def test_seeded_request_batch_1_and_3():
    """The same seeded request alone and in a batch of three: oracle-
    consistent in both, and equal token for token as long as the prefixes
    agree and the oracle's decision margin exceeds the tolerance."""
    name = "tiny"
    eng = _engine(name, seed=4)
    tap = Tap(eng)
    prompts = mo.case_tokens(name, "seeded", (13, 22, 7))
    runs = []
    for batch in (1, 3):
        tap.clear()
        params = [_params(0.7, 4242), _params(1.3), _params(0.0)][:batch]
        seqs = _submit(eng, prompts[:batch], params)
        _drive(eng)
        truth, budget = _check(name, tap, seqs, f"seeded batch-{batch}")
        runs.append((seqs[0], truth.logits[0], budget))
    (a, La, ba), (b, _, _) = runs
    assert a.noise_seed == b.noise_seed == 4242
    n0 = len(a.prompt)
    compared = 0
    for k in range(1, len(a.generated)):
        if a.generated[:k] != b.generated[:k]:
            break
        _, margin = mo.gumbel_ok(La[n0 + k - 1], a.generated[k], 0.7, 4242,
                                 n0 + k, ba.logits_mx)
        if margin > 0:
            assert a.generated[k] == b.generated[k], \
                f"token {k} depends on the batch composition"
            compared += 1
    print(f"seeded request: {compared} unambiguous tokens equal")
