"""The model-level yardstick proved without a GPU (tests/model_oracle.py):
the fp64 oracle agrees with the project's fp32 CPU path, an independent
bf16-staged emulation stays inside every budget the GPU files derive,
planted wiring faults exceed them, and the trajectory check rejects random
tokens."""
import functools

import pytest
import torch

import model_oracle as mo


# ---------------------------------------------------------------------------
# oracle == the fp32 CPU path


@pytest.mark.parametrize("name", mo.CONFIGS)
def test_oracle_matches_fp32_path(name):
    """120 tokens (past tiny-swa's window of 96).  Both run the same
    upcast bf16 weights; the fp32 path accumulates dot products of up to
    1216 terms in float32 (~sqrt(K) 2^-24 each) through 2-3 layers, so rows
    agree to ~1e-6 relative; observed worst rel 2.2e-6 and mx 6.7e-6 over
    the five configs.  The bounds leave roughly 10 x that."""
    seqs = mo.case_tokens(name, "fp32", (120, 7))
    m = mo.upcast_model(name)
    got, truth = mo.reference_run(m, seqs), mo.oracle_forward(m, seqs)
    worst = [0.0, 0.0]
    for g, t in ((got.logits, truth.logits), (got.K, truth.K),
                 (got.V, truth.V)):
        for a, b in zip(g, t):
            rel, mx = mo.row_metrics(a, b)
            worst = [max(worst[0], float(rel.max())),
                     max(worst[1], float(mx.max()))]
    print(f"fp32 path vs oracle {name}: rel {worst[0]:.3g} mx {worst[1]:.3g}")
    assert worst[0] <= 2.5e-5 and worst[1] <= 1.2e-4, worst


# ---------------------------------------------------------------------------
# the second emulation inside every budget


@pytest.mark.parametrize("name", mo.CONFIGS)
def test_second_emulation_inside_budgets(name):
    """emulate_chain rounds at the fused chain's points only and uses bf16
    P; it must fit the budgets measured from the reference run at every
    case the GPU forward file uses.  Worst ratio observed: see
    docs/KERNELS.md."""
    m = mo.cpu_model(name)
    worst = 0.0
    for tag, lens in mo.forward_cases():
        seqs, truth, budget = mo.truth_of(name, tag, lens)
        r = budget.fresh().hold_obs(mo.emulate_chain(m, seqs), truth,
                                    f"{name} {tag}")
        worst = max(worst, max(r.values()))
    print(f"second emulation {name}: worst ratio {worst:.3f}")
    assert worst <= 1.0


def test_reference_budget_size():
    """The budgets are of the size the method assumes: logits rel of the
    reference run ~1e-2, far below the O(1) a wiring fault causes."""
    for name in ("tiny", "tiny-qwen"):
        _, _, b = mo.truth_of(name, "one120", (120,))
        rel, mx = b.lim["logits"]
        assert 0.004 < rel < 0.06 and 0.01 < mx < 0.25, (name, rel, mx)


# ---------------------------------------------------------------------------
# mutants


def _exceeds(budget, got, truth, rows=None):
    """Some observable of the rows [(seq, pos)] (default: all) is past its
    budget."""
    worst = 0.0
    for s in range(len(truth.logits)):
        n = truth.logits[s].shape[0]
        pick = [p for q, p in rows if q == s] if rows else list(range(n))
        if not pick:
            continue
        pick = torch.tensor(pick)
        worst = max(worst, budget.ratio("logits", got.logits[s][pick],
                                        truth.logits[s][pick]))
        for li in range(truth.K[s].shape[0]):
            worst = max(worst,
                        budget.ratio(("K", li), got.K[s][li][pick],
                                     truth.K[s][li][pick]),
                        budget.ratio(("V", li), got.V[s][li][pick],
                                     truth.V[s][li][pick]))
    return worst


def _mutant(name, tag, lens, mut):
    seqs, truth, budget = mo.truth_of(name, tag, lens)
    return mo.oracle_forward(mo.cpu_model(name), seqs, mut), truth, budget


def test_mutant_rope_position_off_by_one():
    def rp(si, pos):
        pos = pos.clone()
        if si == 1:
            pos[17] += 1
        return pos
    got, truth, b = _mutant("tiny", "varlen", (1, 31, 33, 65),
                            {"rope_pos": rp})
    assert _exceeds(b, got, truth, [(1, 17)]) > 1.0
    assert _exceeds(b, got, truth, [(2, 17)]) == 0.0


@pytest.mark.parametrize("layer", (0, 1, 2))
def test_mutant_residual_add_dropped(layer):
    got, truth, b = _mutant("qwen-mini", "decode5",
                            tuple(c + 1 for c in mo.decode_ctx(5)),
                            {"drop_res": layer})
    last = [(s, t.shape[0] - 1) for s, t in enumerate(truth.logits)]
    for row in last:
        assert _exceeds(b, got, truth, [row]) > 1.0


@pytest.mark.parametrize("name,tiles", (("tiny", 1), ("qwen-mini", 1),
                                        ("qwen-mini", 21)))
def test_mutant_rstd_from_wrong_tile_count(name, tiles):
    """The consumer of the o epilogue's partials sums `tiles` of them
    instead of hidden / 32 (nt = 1 kept after the first layer; one tile
    short)."""
    got, truth, b = _mutant(name, "decode5",
                            tuple(c + 1 for c in mo.decode_ctx(5)),
                            {"rstd_tiles": (1, tiles)})
    for s, t in enumerate(truth.logits):
        assert _exceeds(b, got, truth, [(s, t.shape[0] - 1)]) > 1.0


@pytest.mark.parametrize("name", ("tiny-qwen", "qwen-mini"))
def test_mutant_bias_left_unreordered(name):
    """bqkv handed to the pair-ordered pack instead of bqkv_rp: output
    element order[j] receives bias[j]."""
    from ollamamq_amd.ops import hip
    cfg = mo.config(name)
    order = hip.qkv_rope_order(cfg.n_heads, cfg.n_kv_heads)
    inv = [0] * len(order)
    for j, o in enumerate(order):
        inv[o] = j
    assert inv != list(range(len(order)))
    got, truth, b = _mutant(name, "decode5",
                            tuple(c + 1 for c in mo.decode_ctx(5)),
                            {"bias_order": inv})
    for s, t in enumerate(truth.logits):
        assert _exceeds(b, got, truth, [(s, t.shape[0] - 1)]) > 1.0


def test_mutant_window_ignored():
    got, truth, b = _mutant("tiny-swa", "one120", (120,), {"window": 0})
    W = mo.config("tiny-swa").sliding_window
    assert _exceeds(b, got, truth, [(0, p) for p in range(W)]) == 0.0
    for p in (W + 3, 110, 119):
        assert _exceeds(b, got, truth, [(0, p)]) > 1.0


def test_mutant_logits_idx_off_by_one():
    seqs, truth, b = mo.truth_of("tiny", "varlen", (1, 31, 33, 65))
    for s in (1, 2, 3):
        n = truth.logits[s].shape[0]
        r = b.ratio("logits", truth.logits[s][n - 2], truth.logits[s][n - 1])
        assert r > 1.0


def test_mutant_decode_misses_own_key():
    lens = tuple(c + 1 for c in mo.decode_ctx(5))
    for s, n in enumerate(lens):
        got, truth, b = _mutant("tiny", "decode5", lens,
                                {"no_self": (s, n - 1)})
        assert _exceeds(b, got, truth, [(s, n - 1)]) > 1.0


def test_mutant_continued_chunk_restarts_positions():
    def rp(si, pos):
        return torch.where(pos >= 16, pos - 16, pos)
    got, truth, b = _mutant("tiny", "chunks", (39,), {"rope_pos": rp})
    assert _exceeds(b, got, truth, [(0, p) for p in range(16)]) == 0.0
    for p in range(17, 39):
        assert _exceeds(b, got, truth, [(0, p)]) > 1.0


# ---------------------------------------------------------------------------
# power of the trajectory check


@functools.lru_cache(maxsize=None)
def _greedy_trajectory(name, n_prompt=12, n_gen=48):
    m = mo.cpu_model(name)
    seq = mo.case_tokens(name, "traj", (n_prompt,))[0]
    for _ in range(n_gen):
        L = mo.oracle_forward(m, [seq]).logits[0][-1]
        seq = seq + [int(L.argmax())]
    truth = mo.oracle_forward(m, [seq])
    return seq, truth, mo.Budget(mo.reference_run(m, [seq]), truth)


@pytest.mark.parametrize("name", ("tiny", "qwen-mini"))
def test_trajectory_check_rejects_random_tokens(name):
    """Every generated token of an oracle-greedy trajectory passes; each
    replaced by random ones fails in >= 99 % of the draws."""
    n_prompt = 12
    seq, truth, b = _greedy_trajectory(name, n_prompt)
    V = mo.config(name).vocab
    g = torch.Generator().manual_seed(3)
    fails = total = 0
    for p in range(n_prompt, len(seq)):
        L = truth.logits[0][p - 1]
        assert mo.greedy_ok(L, seq[p], b.logits_mx)
        for t in torch.randint(0, V, (40,), generator=g).tolist():
            if t == seq[p]:
                continue
            total += 1
            fails += not mo.greedy_ok(L, t, b.logits_mx)
    print(f"trajectory power {name}: {fails}/{total} random tokens fail")
    assert fails >= 0.99 * total


def test_gumbel_check_rejects_random_tokens():
    """The same for emulated Gumbel rows: the oracle's own pick passes,
    random picks fail in >= 99 % of the draws."""
    seq, truth, b = _greedy_trajectory("tiny")
    V = mo.config("tiny").vocab
    g = torch.Generator().manual_seed(4)
    fails = total = 0
    for p in range(12, len(seq)):
        L = truth.logits[0][p - 1]
        for T in (0.7, 1.3):
            s = mo.gumbel_margin(L, T, 99, p)
            assert mo.gumbel_ok(L, int(s.argmax()), T, 99, p,
                                b.logits_mx)[0]
            for t in torch.randint(0, V, (20,), generator=g).tolist():
                if t == int(s.argmax()):
                    continue
                total += 1
                fails += not mo.gumbel_ok(L, t, T, 99, p, b.logits_mx)[0]
    assert fails >= 0.99 * total
