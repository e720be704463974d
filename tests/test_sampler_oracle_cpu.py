"""The sampler oracle (tests/sampler_oracle.py) proved on the CPU: the fp32
reference sampler is held to it through the multinomial capture, the
budgets the GPU tests use are measured here, the oracle is cross-checked
against a naive loop and against deliberate mutants of itself, and the
engine's request-seed contract is run through the CPU engine."""
import numpy as np
import pytest
import torch

import sampler_oracle as so
from ollamamq_amd.ops import reference as ref
from ollamamq_amd.models import LlamaModel, PRESETS
from ollamamq_amd.engine import LlamaEngine, PagedKVCache, GenParams
from ollamamq_amd.engine import engine as engine_mod

PLANTS = ("first", "last", "interior")


def _hold(sample_fn, c, plant, mutant=None, row0=False):
    """Rows of the case that miss the (possibly mutated) oracle."""
    bud, gamma_p, _, _ = so.budget(c["name"])
    toks, seen, widths = so.run_captured(sample_fn, c, plant)
    bad, worst, amb = [], 0.0, 0
    for r in range(c["logits"].shape[0]):
        try:
            ratio, a = so.check_row(c, r, toks[r], seen.get(r), bud, gamma_p,
                                    mutant=mutant, T0=row0)
            worst, amb = max(worst, ratio), amb + a
        except AssertionError as e:
            bad.append((r, str(e)))
    return bad, worst, amb


@pytest.mark.parametrize("name", so.case_names())
def test_reference_sampler_holds_the_oracle(name):
    c = so.case(name)
    bud, gamma_p, err, cum_err = so.budget(name)
    print(f"BUDGET {name} rel {bud:.3e} (reference {err:.3e}) "
          f"gamma_p {gamma_p:.3e} (cumsum {cum_err:.3e})")
    margins = [so.boundary_margin(so.filtered_distribution(
        c["logits"][r], c["T"][r], c["top_k"][r], c["top_p"][r]))
        for r in range(c["logits"].shape[0])]
    print(f"MARGIN {name} smallest {min(margins):.3e}")
    for plant in PLANTS:
        bad, worst, amb = _hold(ref.sample, c, plant)
        assert not bad, bad
        assert amb == 0, f"{name}: {amb} ambiguous rows for the reference"
        assert worst <= 0.25 + 1e-12 or bud == so.P_FLOOR


@pytest.mark.parametrize("name", so.case_names())
def test_vectorised_oracle_equals_naive_loop(name):
    c = so.case(name)
    B, V = c["logits"].shape
    rows = range(B) if V <= 4104 else range(min(B, 2))
    for r in rows:
        d = so.filtered_distribution(c["logits"][r], c["T"][r],
                                     c["top_k"][r], c["top_p"][r])
        n, kept = so.naive_distribution(c["logits"][r], c["T"][r],
                                        c["top_k"][r], c["top_p"][r])
        if d.greedy:
            assert n == d.token == int(np.argmax(
                c["logits"][r].double().numpy()))
            continue
        assert n == d.n, (name, r, n, d.n)
        assert np.abs(np.asarray(kept) - d.kept).max() <= 1e-12


def test_greedy_is_numpy_lowest_index_argmax():
    c = so.case("v4104-fast-greedy")
    toks, _, _ = so.run_captured(ref.sample, c, "first")
    l = c["logits"].double().numpy()
    assert toks[1] == int(np.argmax(l[1])) == 7
    assert toks[4] == int(np.argmax(l[4])) == 3


def test_fast_path_flags():
    flags = {n: so.fast_path(so.case(n)) for n in so.case_names()}
    assert flags["v4104-fast"] and flags["v4104-fast-greedy"]
    assert flags["v4104-ties"] and flags["v128256-fast"]
    assert flags["v520-cold"]
    assert flags["v520-topk-capped"] and flags["v520-topp-capped"]
    assert not flags["v4104-nucleus"] and not flags["v520-topk-differs"]
    assert not flags["v128256-sort"] and not flags["v520-temp-only"]


# mutant -> (case at which the comparison must fail, rows it touches)
MUTANTS = {
    "cum_lt_p": ("v520-topp-differs", None),
    "topk_off_by_one": ("v520-topk-differs", None),
    "row0_params": ("v520-topk-differs", None),
    "temp_after_cut": ("v520-topp-differs", None),
    "mass_top256": ("v4104-nucleus", None),
    "rank0_not_forced": ("v520-topp-differs", (8,)),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_oracle_mutants_fail_only_where_they_bite(mutant):
    name, rows = MUTANTS[mutant]
    c = so.case(name)
    B = c["logits"].shape[0]
    gamma_p = so.budget(name)[1]
    kw = dict(row0=True) if mutant == "row0_params" else dict(mutant=mutant)
    # the rows the mutant touches: its distribution differs from the true
    touched = []
    for r in range(B):
        src = 0 if mutant == "row0_params" else r
        a = so.filtered_distribution(c["logits"][r], c["T"][r],
                                     c["top_k"][r], c["top_p"][r])
        b = so.filtered_distribution(
            c["logits"][r], c["T"][src], c["top_k"][src], c["top_p"][src],
            mutant=None if mutant == "row0_params" else mutant)
        if a.greedy != b.greedy:
            touched.append(r)
        elif not a.greedy and a.n != b.n:
            # a count one off hides behind a mutant's own ambiguous cut
            if abs(a.n - b.n) > 1 or so.boundary_margin(b) >= gamma_p:
                touched.append(r)
        elif not a.greedy and np.abs(a.kept - b.kept).max() > 1e-9:
            touched.append(r)
    assert touched and len(touched) < B, (mutant, touched)
    if rows is not None:
        assert tuple(touched) == rows
    bad, _, _ = _hold(ref.sample, c, "last", **kw)
    assert [r for r, _ in bad] == touched, (mutant, bad, touched)


def test_parent_tail_nucleus_is_not_the_reference():
    """V = 4104, T = 1, top_p = 0.5: mass measured on the top-256
    renormalised keeps a fraction of the true nucleus."""
    c = so.case("v4104-nucleus")
    true = so.filtered_distribution(c["logits"][0], 1.0, 0, 0.5)
    cut = so.filtered_distribution(c["logits"][0], 1.0, 0, 0.5,
                                   mutant="mass_top256")
    print(f"NUCLEUS true {true.n} top-256-renormalised {cut.n} "
          f"top-256 mass {true.probs[:256].sum():.3f}")
    assert true.n > 256 > cut.n


# ---------------------------------------------------------------------------
# request-seed contract through the CPU engine

SEEDS = (0, 1, -1, 2 ** 31, 2 ** 44, 2 ** 50, 2 ** 63 - 1, 2 ** 63,
         2 ** 64 - 1, 2 ** 64 + 5, -2 ** 63, -2 ** 63 - 1, -2 ** 70)


@pytest.fixture(scope="module")
def model():
    return LlamaModel(PRESETS["tiny"], device="cpu", dtype=torch.float32,
                      seed=7)


def _engine(model):
    cfg = model.cfg
    kv = PagedKVCache.for_model(cfg, n_pages=64, max_slots=4,
                                max_ctx=cfg.max_ctx)
    return LlamaEngine(model, kv, max_batch=4)


def _run(model, params, prompts):
    eng = _engine(model)
    seqs = [eng.seqs[eng.submit(list(p), g)] for p, g in zip(prompts, params)]
    for _ in range(200):
        eng.step()
        if not eng.has_work():
            break
    assert not eng.has_work(), "engine did not drain"
    return seqs


P_SAMPLED, P_GREEDY = [5, 9, 2, 7, 1], [3, 1, 4, 1, 5, 9]


@pytest.fixture(scope="module")
def greedy_solo(model):
    return _run(model, [GenParams(max_tokens=6)], [P_GREEDY])[0].generated


@pytest.mark.parametrize("seed", SEEDS)
def test_any_int_seed_drains_and_reproduces(seed, model, greedy_solo):
    def sampled():
        return GenParams(max_tokens=6, temperature=0.8, seed=seed)
    a = _run(model, [sampled()], [P_SAMPLED])[0]
    b = _run(model, [sampled()], [P_SAMPLED])[0]
    assert len(a.generated) == 6 and a.generated == b.generated
    assert -2 ** 63 <= a.noise_seed < 2 ** 63
    assert a.noise_seed % 2 ** 64 == seed % 2 ** 64
    pair = _run(model, [sampled(), GenParams(max_tokens=6)],
                [P_SAMPLED, P_GREEDY])
    assert pair[0].generated == a.generated
    assert pair[1].generated == greedy_solo


def test_host_seed_key():
    key = engine_mod.host_seed_key
    keys = {}
    for s in SEEDS + (2 ** 44 + 1, 2 ** 45, 2 ** 62, 3 << 43):
        for i in (0, 1, 7, 1 << 20, (1 << 20) + 7, 4095):
            k = key(s, i)
            assert 0 <= k < 2 ** 63
            torch.Generator().manual_seed(k)
            keys.setdefault(k, set()).add((s % 2 ** 64, i))
    assert all(len(v) == 1 for v in keys.values()), \
        [v for v in keys.values() if len(v) > 1]
    # seeds that differ only above bit 43
    assert len({key(1, 5), key(1 + 2 ** 44, 5), key(1 + 2 ** 60, 5)}) == 3
    # the parent's (seed << 20) ^ index collides here by construction
    for s, i in ((6, 9), (2 ** 40, 0), (12345, 1 << 20)):
        assert key(s, i) != key(s ^ 1, i ^ (1 << 20))
    # reduced mod 2^64
    assert key(2 ** 64 + 5, 3) == key(5, 3) and key(-1, 3) == key(2 ** 64 - 1, 3)
