"""Logit penalties on the CPU: the fp64 oracle against a naive second
implementation, ops.reference.penalize_logits against the oracle at every
shape the GPU file uses, the oracle's mutants, the engine's penalised
paths on the fp32 CPU model, and the wire parsing.

Worst real-tier ratio of the fp32, round-once reference against the budget
2^-7 |truth| + 2^-8 rms(row): 0.422 at V64-B6-real (one correct bf16
rounding can use half of the relative term; printed as RATIO by
test_reference_matches_oracle)."""
import json
import math
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import pen_oracle as po
from ollamamq_amd.engine.engine import f32
from ollamamq_amd.ops import reference as ref

CASES = po.cases()
IDS = [po.case_id(k) for k in CASES]


# ---------------------------------------------------------------------------
# 1. oracle against the naive implementation


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_oracle_matches_naive(key):
    c = po.make_case(*key)
    x, touched, h = po.truth(key)
    nx, ntouched, nh = po.naive(*(c[a] for a in po.ARGS))
    assert h.tolist() == nh
    for b in range(key[1]):
        assert set(np.nonzero(touched[b])[0].tolist()) == ntouched[b], b
    err = np.abs(x - np.asarray(nx, dtype=np.float64))
    assert float(err.max()) <= 1e-12


def test_cases_cover_the_edges():
    """The shared cases reach what they are meant to: 150 adds on one cell,
    ids 0 and V-1 touched, ignored ids inside a window, both kinds of
    inactive row, rows with and without append, every L and n."""
    seen_L, seen_n, most = set(), set(), 0
    first = last = bad = off = neutral = app = noapp = False
    for key in CASES:
        c = po.make_case(*key)
        V = key[0]
        _, touched, h = po.truth(key)
        act = po.active_rows(c)
        first |= bool(touched[:, 0].any())
        last |= bool(touched[:, V - 1].any())
        for b in range(key[1]):
            L, n = int(c["lens"][b]), int(c["last_n"][b])
            seen_L.add(L)
            seen_n.add(n)
            app |= int(c["tok"][b]) >= 0
            noapp |= int(c["tok"][b]) < 0
            off |= n == 0
            neutral |= n != 0 and not bool(act[b])
            if not act[b]:
                continue
            w = L if (n < 0 or n > L) else n
            win = h[int(c["slot"][b]), L - w:L].astype(np.int64)
            bad |= bool(((win < 0) | (win >= V)).any())
            win = win[(win >= 0) & (win < V)]
            if win.size:
                most = max(most, int(np.bincount(win).max()))
    assert seen_L == set(po.LENS) and seen_n == set(po.LAST_NS)
    assert most == 150
    assert first and last and bad and off and neutral and app and noapp


# ---------------------------------------------------------------------------
# 2. the fp32 reference against the oracle


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_reference_matches_oracle(key):
    c = po.make_case(*key)
    logits, hist = c["logits"].clone(), c["hist"].clone()
    out = ref.penalize_logits(logits, hist, *(c[a] for a in po.ARGS[2:]))
    assert out is logits
    r = po.check_against_oracle(key, logits, hist, "reference")
    print(f"RATIO penalty-reference {po.case_id(key)} {r:.3f}")


# ---------------------------------------------------------------------------
# 3. mutants of the oracle


def _may_differ(c, mut, h_after):
    """Rows a mutant is allowed to change."""
    act = po.active_rows(c)
    L, n = c["lens"], c["last_n"]
    w = torch.where((n < 0) | (n > L), L, n)
    if mut == "lo_plus":
        return act & (w >= 1)
    if mut == "shift":
        return act & (L >= 1)
    if mut == "no_prompt":
        return act & (L - w < c["prompt_len"])
    if mut == "cap":
        return act & (c["fp"] != 0)
    if mut == "rp_after":
        return act & (c["rp"] != 1)
    if mut == "no_append":
        return act & (c["tok"] >= 0)
    raise KeyError(mut)


@pytest.mark.parametrize("mut", po.MUTANTS)
def test_oracle_mutant_fails_on_its_rows_only(mut):
    hit = 0
    for key in CASES:
        if key[0] > 4104:
            continue
        c = po.make_case(*key)
        x, _, h = po.truth(key)
        mx, _, mh = po.oracle(*(c[a] for a in po.ARGS), mut=mut,
                              prompt_len=c["prompt_len"])
        assert np.array_equal(h, mh)
        rows = torch.from_numpy((x != mx).any(axis=1))
        allowed = _may_differ(c, mut, h)
        assert not bool((rows & ~allowed).any()), (mut, po.case_id(key))
        # what a test would see: the real-tier budget, the exact equality
        if bool(rows.any()):
            hit += 1
            if key[2] == "exact":
                assert not np.array_equal(mx, x)
    assert hit >= 4, f"mutant {mut} changed {hit} cases only"


def test_mutants_miss_the_budget():
    """Each mutant is not merely different but outside the real-tier
    budget, or unequal in the exact tier, on some case: a test holding
    that budget catches it."""
    for mut in po.MUTANTS:
        caught = False
        for key in CASES:
            if key[0] > 520 or caught:
                continue
            c = po.make_case(*key)
            x, _, _ = po.truth(key)
            mx, _, _ = po.oracle(*(c[a] for a in po.ARGS), mut=mut,
                                 prompt_len=c["prompt_len"])
            t, g = torch.from_numpy(x), torch.from_numpy(mx)
            rms = t.pow(2).mean(-1, keepdim=True).sqrt()
            caught = bool(((g - t).abs()
                           > t.abs() * 2.0 ** -7 + rms * 2.0 ** -8).any())
        assert caught, mut


def test_zero_logit_branch():
    """`x < 0` for `x <= 0` with a planted zero logit: at x = 0 both
    branches give 0 * rp = 0 / rp = 0 for every finite rp > 0, so the two
    spellings compute the same function and no output can tell them apart.
    The planted zero is checked to take the penalty (0 - (c fp + pp)) under
    both, and the mutant to agree with the oracle on every case."""
    V = 64
    logits = torch.zeros((1, V), dtype=torch.bfloat16)
    logits[0, 5] = -0.0
    hist = torch.full((po.MAX_SLOTS, po.MAX_CTX), -1, dtype=torch.int32)
    hist[3, :4] = torch.tensor([7, 7, 5, 9], dtype=torch.int32)
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)        # noqa: E731
    f32 = lambda *a: torch.tensor(a, dtype=torch.float32)      # noqa: E731
    args = (logits, hist, i32(3), i32(4), i32(-1), i32(-1), f32(2.0),
            f32(0.5), f32(0.25))
    for mut in (None, "lt"):
        x, touched, _ = po.oracle(*args, mut=mut)
        assert sorted(np.nonzero(touched[0])[0].tolist()) == [5, 7, 9]
        assert x[0, 7] == -1.0 and x[0, 5] == -0.75 and x[0, 9] == -0.75
    for key in CASES:
        if key[0] > 4104:
            continue
        c = po.make_case(*key)
        mx, _, _ = po.oracle(*(c[a] for a in po.ARGS), mut="lt")
        assert np.array_equal(mx, po.truth(key)[0])


# ---------------------------------------------------------------------------
# 4. the CPU engine on `tiny`


def make_engine(max_slots=6, prefill_chunk=2048, preset="tiny"):
    from ollamamq_amd.engine import LlamaEngine, PagedKVCache
    from ollamamq_amd.models import LlamaModel, PRESETS
    cfg = PRESETS[preset]
    model = LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=7)
    kv = PagedKVCache.for_model(cfg, n_pages=128, max_slots=max_slots,
                                max_ctx=256)
    return LlamaEngine(model, kv, max_batch=max_slots,
                       prefill_chunk=prefill_chunk)


def run_all(eng, max_steps=600):
    for _ in range(max_steps):
        eng.step()
        if not eng.has_work():
            break
    assert not eng.has_work(), "engine did not drain"


def presence(n=-1, max_tokens=40, **kw):
    from ollamamq_amd.engine import GenParams
    return GenParams(max_tokens=max_tokens, presence_penalty=1000.0,
                     repeat_last_n=n, **kw)


def assert_distinct(seq, V=512):
    """presence_penalty = 1000 over the whole sequence: no generated token
    repeats another or a prompt token (the logits of a random-init model
    are a few units wide, and fewer than V tokens are in play)."""
    all_t = seq.prompt + seq.generated
    assert len(all_t) < V
    assert len(set(seq.generated)) == len(seq.generated), seq.generated
    assert not set(seq.generated) & set(seq.prompt), seq.generated


def assert_window_distinct(seq, n):
    all_t = seq.prompt + seq.generated
    for i in range(len(seq.prompt), len(all_t)):
        assert all_t[i] not in all_t[max(0, i - n):i], (i, all_t)


PROMPT = [5, 9, 2, 7, 9, 11, 300, 4, 4, 17]


def _run_one(params, prompt=PROMPT, **kw):
    eng = make_engine(**kw)
    seq = eng.seqs[eng.submit(list(prompt), params)]
    run_all(eng)
    return eng, seq


def test_engine_presence_makes_tokens_distinct():
    from ollamamq_amd.engine import GenParams
    _, plain = _run_one(GenParams(max_tokens=40))
    # the property is not vacuous: unpenalised, this model repeats itself
    assert len(set(plain.generated)) < len(plain.generated) \
        or set(plain.generated) & set(PROMPT)
    eng, seq = _run_one(presence())
    assert len(seq.generated) == 40
    assert_distinct(seq)
    assert eng._hist is not None


def test_engine_window_of_four():
    _, seq = _run_one(presence(n=4))
    assert len(seq.generated) == 40
    assert_window_distinct(seq, 4)


def test_engine_inactive_requests_unchanged():
    from ollamamq_amd.engine import GenParams
    _, plain = _run_one(GenParams(max_tokens=24))
    eng, explicit = _run_one(GenParams(
        max_tokens=24, repeat_penalty=1.0, repeat_last_n=64,
        presence_penalty=0.0, frequency_penalty=0.0))
    assert explicit.generated == plain.generated
    assert eng._hist is None and eng._counts is None
    eng, off = _run_one(GenParams(max_tokens=24, repeat_penalty=5.0,
                                  repeat_last_n=0))
    assert off.generated == plain.generated
    assert eng._hist is None


def test_engine_repeat_penalty_changes_tokens():
    """repeat_penalty alone (Ollama's 1.1 is too weak to show on every
    model; 5.0 is not) differs from the plain run and is deterministic."""
    from ollamamq_amd.engine import GenParams
    _, plain = _run_one(GenParams(max_tokens=24))
    _, a = _run_one(GenParams(max_tokens=24, repeat_penalty=5.0))
    _, b = _run_one(GenParams(max_tokens=24, repeat_penalty=5.0))
    assert a.generated == b.generated != plain.generated


def test_engine_neighbour_untouched():
    from ollamamq_amd.engine import GenParams
    other = [3, 1, 4, 1, 5, 9, 2, 6]
    _, solo = _run_one(GenParams(max_tokens=30), prompt=other)
    eng = make_engine()
    pen = eng.seqs[eng.submit(list(PROMPT), presence())]
    nb = eng.seqs[eng.submit(list(other), GenParams(max_tokens=30))]
    run_all(eng)
    assert nb.generated == solo.generated
    assert_distinct(pen)


def test_engine_chunked_late_and_slot_reuse():
    """prefill_chunk = 16 (a 40-token prompt takes three chunks), a
    penalised sequence admitted while others decode, and a slot reused
    after a finished penalised sequence."""
    from ollamamq_amd.engine import GenParams
    g = torch.Generator().manual_seed(5)
    long_p = torch.randint(0, 512, (40,), generator=g).tolist()
    eng = make_engine(max_slots=2, prefill_chunk=16)
    a = eng.seqs[eng.submit(long_p, presence(max_tokens=30))]
    b = eng.seqs[eng.submit([8, 8, 8], GenParams(max_tokens=50))]
    for _ in range(12):
        eng.step()
    # both slots busy: c waits, then takes the slot a leaves
    c = eng.seqs[eng.submit(long_p[::-1], presence(max_tokens=30))]
    slot_a = a.slot
    seen = set()
    for _ in range(600):
        eng.step()
        if c.slot >= 0:
            seen.add(c.slot)
        if not eng.has_work():
            break
    assert not eng.has_work()
    assert seen == {slot_a}, (seen, slot_a)
    for s in (a, c):
        assert len(s.generated) == 30
        assert_distinct(s)
    assert len(b.generated) == 50
    # late admission into a running batch, chunked
    eng = make_engine(max_slots=4, prefill_chunk=16)
    a = eng.seqs[eng.submit(list(PROMPT), presence())]
    for _ in range(6):
        eng.step()
    d = eng.seqs[eng.submit(long_p, presence(n=4, max_tokens=30))]
    run_all(eng)
    assert_distinct(a)
    assert_window_distinct(d, 4)


# ---------------------------------------------------------------------------
# 5. wire


def _params(body, openai=False):
    from ollamamq_amd.engine.tokenizer import ByteTokenizer
    from ollamamq_amd.engine.worker import _params_from_body
    return _params_from_body(body, ByteTokenizer(256), openai)


def test_wire_reads_both_spellings():
    p = _params({"options": {"repeat_penalty": 1.3, "repeat_last_n": -1,
                             "presence_penalty": 0.5,
                             "frequency_penalty": -0.25}})
    # the parameters come back rounded to fp32, what the kernel computes in
    assert (p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
            p.frequency_penalty) == (f32(1.3), -1, 0.5, -0.25)
    assert p.penalty_active
    p = _params({"presence_penalty": 1.5, "frequency_penalty": 0.75}, True)
    assert (p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
            p.frequency_penalty) == (1.0, 64, 1.5, 0.75)
    # the body wins over options, as for temperature
    p = _params({"presence_penalty": 2.0,
                 "options": {"presence_penalty": 0.5}})
    assert p.presence_penalty == 2.0
    # nothing named: today's path
    p = _params({"options": {"temperature": 0.7}})
    assert (p.repeat_penalty, p.repeat_last_n, p.presence_penalty,
            p.frequency_penalty) == (1.0, 64, 0.0, 0.0)
    assert not p.penalty_active
    assert not _params({"options": {"repeat_penalty": 1.0}}).penalty_active
    assert not _params({"options": {"repeat_penalty": 1.5,
                                    "repeat_last_n": 0}}).penalty_active
    # numeric strings are read alike in all four
    p = _params({"options": {"repeat_penalty": "1.5", "repeat_last_n": "8",
                             "presence_penalty": "0.5"}})
    assert (p.repeat_penalty, p.repeat_last_n, p.presence_penalty) \
        == (1.5, 8, 0.5)
    assert _params({"options": {"repeat_last_n": 64.0}}).repeat_last_n == 64
    # host and kernel judge "active" on the same fp32 value: this is 1.0f
    p = _params({"options": {"repeat_penalty": 1.00000000001}})
    assert p.repeat_penalty == 1.0 and not p.penalty_active
    from ollamamq_amd.engine import GenParams
    assert not GenParams(repeat_penalty=1.00000000001).penalty_active
    assert GenParams(repeat_penalty=1.000001).penalty_active


@pytest.mark.parametrize("n", [2 ** 31 - 1, 2 ** 31, 3000000000, 1e30,
                               10 ** 30])
def test_wire_and_engine_take_a_huge_window(n):
    """n larger than the sequence is clamped to it, however large: past the
    int32 range it is cut at the wire and again where the engine packs it,
    and the tokens are those of the whole-sequence window."""
    from ollamamq_amd.engine import GenParams
    p = _params({"options": {"repeat_last_n": n, "presence_penalty": 1000}})
    assert p.repeat_last_n == 2 ** 31 - 1 and p.penalty_active
    _, whole = _run_one(presence(n=-1, max_tokens=12))
    # straight into the engine, unclamped, beside an unpenalised neighbour
    eng = make_engine()
    seq = eng.seqs[eng.submit(list(PROMPT), GenParams(
        max_tokens=12, presence_penalty=1000.0, repeat_last_n=int(n)))]
    nb = eng.seqs[eng.submit([3, 1, 4], GenParams(max_tokens=12))]
    run_all(eng)
    assert seq.generated == whole.generated
    assert len(nb.generated) == 12 and nb.finish_reason == "length"
    assert_distinct(seq)


@pytest.mark.parametrize("opts", [
    {"repeat_penalty": 0}, {"repeat_penalty": -1},
    {"repeat_penalty": float("nan")}, {"repeat_penalty": float("inf")},
    {"repeat_penalty": "x"}, {"repeat_last_n": -2}, {"repeat_last_n": 1.5},
    {"presence_penalty": float("inf")},
    {"frequency_penalty": float("nan")},
    # 1e400 in a JSON body parses to inf
    {"repeat_last_n": float("inf")}, {"repeat_last_n": float("nan")},
    {"repeat_last_n": "1.5"}, {"repeat_last_n": [4]},
    {"repeat_last_n": True},
    # zero or infinite once rounded to fp32
    {"repeat_penalty": 1e-60}, {"repeat_penalty": 1e300},
    {"presence_penalty": 1e39}, {"frequency_penalty": -1e39}], ids=str)
def test_wire_rejects(opts):
    # the two exception types the request path turns into a 400
    with pytest.raises((ValueError, TypeError)):
        _params({"options": opts})
    # and from the JSON text a client sends, where 1e400 reads as inf
    with pytest.raises((ValueError, TypeError)):
        _params(json.loads(json.dumps({"options": opts})))
    if "repeat_penalty" not in opts and "repeat_last_n" not in opts:
        with pytest.raises((ValueError, TypeError)):
            _params(opts, True)


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "ollamamq_amd", "csrc", "dispatcher",
                   "ollamamq-server")


@pytest.fixture(scope="module")
def stack(tmp_path_factory, sock_dir_module):
    """Dispatcher -> UDS -> CPU worker, as tests/test_worker_stack.py."""
    import httpx
    if not os.path.exists(BIN):
        subprocess.run([sys.executable, "-m", "ollamamq_amd.build"],
                       check=True)
    tmp = tmp_path_factory.mktemp("penstack")
    sock = os.path.join(sock_dir_module, "wp.sock")
    worker = subprocess.Popen(
        [sys.executable, "-m", "ollamamq_amd.engine.worker",
         "--socket", sock, "--model", "tiny-cpu", "--max-ctx", "256",
         "--max-batch", "4"],
        cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    server = None
    try:
        t0 = time.time()
        up = False
        while time.time() - t0 < 60 and not up:
            if os.path.exists(sock):
                s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
                try:
                    s.connect(sock)
                    up = True
                except OSError:
                    pass
                finally:
                    s.close()
            if not up:
                time.sleep(0.2)
        assert up, "worker did not come up"
        server = subprocess.Popen(
            [BIN, "--no-tui", "-p", "0", "-w", sock,
             "-c", os.path.join(str(tmp), "absent.yaml")],
            stderr=subprocess.PIPE, cwd=str(tmp), text=True)
        line = server.stderr.readline()
        base = f"http://127.0.0.1:{int(line.rsplit(':', 1)[1].split()[0])}"
        deadline = time.time() + 20
        while time.time() < deadline:
            try:
                r = httpx.get(base + "/admin/models").json()
                if r and r[0]["online"]:
                    break
            except Exception:
                pass
            time.sleep(0.2)
        yield base
    finally:
        if server is not None:
            server.terminate()
        worker.terminate()


def test_stack_rejects_zero_repeat_penalty(stack):
    import httpx
    r = httpx.post(stack + "/api/generate",
                   json={"model": "tiny-cpu", "prompt": "abc",
                         "stream": False,
                         "options": {"repeat_penalty": 0}}, timeout=60.0)
    assert r.status_code == 400
    assert "invalid options" in r.json()["error"]


def test_stack_rejects_overflowing_window_text(stack):
    """`1e400` is legal JSON and reads as inf: a clean 400, and a window
    past the int32 range is served."""
    import httpx
    body = ('{"model": "tiny-cpu", "prompt": "abc", "stream": false, '
            '"options": {"repeat_last_n": 1e400, "repeat_penalty": 1.1}}')
    r = httpx.post(stack + "/api/generate", content=body,
                   headers={"Content-Type": "application/json"},
                   timeout=60.0)
    assert r.status_code == 400, r.text
    assert "invalid options" in r.json()["error"]
    r = httpx.post(stack + "/api/generate",
                   json={"model": "tiny-cpu", "prompt": "abc",
                         "stream": False,
                         "options": {"num_predict": 6,
                                     "repeat_last_n": 3000000000,
                                     "repeat_penalty": 1.1}}, timeout=120.0)
    assert r.status_code == 200, r.text
    assert r.json()["eval_count"] == 6


def test_stack_presence_penalty_distinct_tokens(stack):
    """One streamed piece per token and the tokenizer's rendering is
    one-to-one, so distinct pieces are distinct tokens."""
    import httpx
    from ollamamq_amd.engine.tokenizer import ByteTokenizer
    prompt = "abcabc"
    r = httpx.post(stack + "/api/generate",
                   json={"model": "tiny-cpu", "prompt": prompt,
                         "options": {"num_predict": 24,
                                     "presence_penalty": 1000,
                                     "repeat_last_n": -1}}, timeout=120.0)
    assert r.status_code == 200, r.text
    lines = [json.loads(l) for l in r.text.strip().split("\n")]
    assert lines[-1]["done"] is True and lines[-1]["eval_count"] == 24
    pieces = [l["response"] for l in lines[:-1]]
    assert len(pieces) == 24 and len(set(pieces)) == 24, pieces
    tok = ByteTokenizer(256)
    assert not set(pieces) & {tok.decode_one(t) for t in tok.encode(prompt)}
    assert math.isfinite(lines[-1]["eval_duration"])
