"""ops/hip.py candidate_filter, the one top-k/top-p filter behind
hip.sample's fast path and the engine's class-2 tail, held to the fp64
sampler oracle on CPU tensors: through the same multinomial capture and
row check as ref.sample in tests/test_sampler_oracle_cpu.py, on batches of
one logits row whose rows differ only in top_k or only in top_p, beside a
greedy row.  V = 300 leaves mass outside the C = 256 candidates; at V = 40
the candidates are the whole row."""
import pytest
import torch

import sampler_oracle as so
from ollamamq_amd.ops import hip

PLANTS = ("first", "last", "interior")


def _one_row(V, seed, n):
    return so._randn_bf16(1, V, seed).expand(n, V).clone()


def _cases():
    out = []
    for V, seed in ((300, 31), (40, 33)):
        C = min(256, V)
        ks = [1, 2, 5, C - 1, C]
        # only top_k differs (top_p off); the last row is greedy
        out.append(so._case(f"filter-v{V}-topk", _one_row(V, seed, 6),
                            [0.7] * 5 + [0.0], ks + [5], [1.0] * 6))
        # only top_p differs, top_p = 1.0 and 1.5 (off) among them; the
        # last row is greedy
        n = len(so.TOP_PS) + 1
        out.append(so._case(f"filter-v{V}-topp", _one_row(V, seed + 1, n),
                            [1.3] * (n - 1) + [-1.0], [C] * n,
                            list(so.TOP_PS) + [0.5]))
    return out


CASES = {c["name"]: c for c in _cases()}


def _sample_through_filter(seen):
    """A sampler made of candidate_filter and the least around it: the
    kept probabilities to multinomial, the pick gathered to a token, the
    greedy rows' argmax."""
    def fn(logits, temps, top_k, top_p, generator):
        v, idx, p, keep, greedy = hip.candidate_filter(
            logits, temps, top_k, top_p)
        seen.update(v=v, idx=idx, p=p, keep=keep, greedy=greedy)
        pm = p * keep
        pick = torch.multinomial(pm / pm.sum(-1, keepdim=True), 1,
                                 generator=generator).squeeze(1)
        tok = idx.gather(1, pick.unsqueeze(1)).squeeze(1)
        return torch.where(greedy, logits.float().argmax(-1), tok)
    return fn


@pytest.mark.parametrize("name", sorted(CASES))
def test_candidate_filter_holds_the_oracle(name):
    c = CASES[name]
    B, V = c["logits"].shape
    C = min(256, V)
    assert so.fast_path(c)
    bud, gamma_p, err, cum_err = so.case_budget(c)
    print(f"BUDGET {name} rel {bud:.3e} (reference {err:.3e}) "
          f"gamma_p {gamma_p:.3e} (cumsum {cum_err:.3e})")
    for plant in PLANTS:
        out = {}
        toks, seen, widths = so.run_captured(_sample_through_filter(out), c,
                                             plant)
        assert widths == [C]
        amb = 0
        for r in range(B):
            # the kept set, as non-zero probabilities, within check_row's
            # exemptions (a cut closer than gamma_p to top_p, probabilities
            # fp32 may flush) and no others; greedy rows by their token
            ratio, a = so.check_row(c, r, toks[r], seen.get(r), bud, gamma_p)
            amb += a
            d = so.filtered_distribution(c["logits"][r], c["T"][r],
                                         c["top_k"][r], c["top_p"][r])
            if d.greedy:
                assert bool(out["greedy"][r])
                continue
            keep = out["keep"][r]
            n = int(keep.sum())
            assert keep[:n].all(), "kept ranks are a prefix"
            assert n == d.n or (a and abs(n - d.n) == 1), \
                f"{name} row {r}: keeps {n}, oracle {d.n}"
            # raw values in descending order, gathered from their tokens
            v = out["v"][r]
            assert (v[:-1] >= v[1:]).all()
            assert torch.equal(c["logits"][r].float()[out["idx"][r]], v)
            assert v.double().tolist() == d.raw[:C].tolist()
        assert amb == 0, f"{name}: {amb} ambiguous rows"
