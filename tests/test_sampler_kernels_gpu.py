"""k_argmax / k_argmax_part / k_argmax_comb and k_gumbel_part / k_gumbel_comb
against exact expectations from tests/elem_oracle.py.

argmax: planted equal maxima across a thread's rounds, lanes, waves and
slice edges; the numpy lowest-index argmax is the reference.  Gumbel,
counter mode: the noise is the documented function of (seed, ctr, v),
emulated bit for bit on the CPU; the expected token is the fp64 argmax of
l / T - log(-log(u)).  Rows whose fp64 best-to-runner-up gap is at least
elem_oracle.GUMBEL_GAMMA must match exactly, the others must pick one of
the two.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elem_oracle as eo

DEV = "cuda:0"


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


# ---------------------------------------------------------------------------
# argmax


def _argmax_check(hip, rows, expected, B):
    rows_g = rows.to(DEV)
    for idx in eo.batches(rows.shape[0], B):
        ix = torch.tensor(idx)
        out = hip.sample(rows_g[ix.to(DEV)].contiguous(), 0.0, 0, 1.0)
        assert out.shape == (B,)
        got, want = out.cpu().tolist(), expected[ix].tolist()
        assert got == want, \
            [(i, g, w) for i, g, w in zip(idx, got, want) if g != w][:8]


@pytest.mark.parametrize("B", eo.ARGMAX_B)
def test_argmax_planted_ties(B):
    """V = 4104: slices [0, 2048) [2048, 4096) [4096, 4104) for B <= 64,
    [0, 4096) [4096, 4104) at B = 384, one block per row above."""
    rows, expected = eo.argmax_rows(eo.ARGMAX_V)
    _argmax_check(_hip(), rows, expected, B)


@pytest.mark.parametrize("B", eo.ARGMAX_BIG_B)
def test_argmax_planted_ties_llama3_vocab(B):
    rows, expected = eo.argmax_rows(eo.ARGMAX_BIG_V, ties_only=True)
    _argmax_check(_hip(), rows, expected, B)


@pytest.mark.parametrize("V", eo.ARGMAX_SMALL_V + eo.ARGMAX_ODD_V)
def test_argmax_small_and_odd_vocab(V):
    """V = 7, 513, 2049 collapse the slices to one or two (V = 7 is below
    the slice count); none is a multiple of 8, so the single maximum at
    V - 1 sits in a scalar tail (4101: the tail of the third slice).
    65541 = 32 x 2048 + 5: V / 32 lies just above a multiple of 2048, where
    a slice length rounded from floor(V / 32) stops 5 tokens short."""
    assert V % 8
    rows, expected = eo.argmax_rows(V)
    for B in (1, 32, 385):
        _argmax_check(_hip(), rows, expected, B)


# ---------------------------------------------------------------------------
# gumbel, counter mode


@pytest.mark.parametrize("B,V", eo.GUMBEL_CASES)
def test_gumbel_counter_mode_matches_emulation(B, V):
    hip = _hip()
    logits, temps, seeds, ctrs = eo.gumbel_case(B, V)
    best, runner, gap, _ = eo.gumbel_expected(B, V)
    args = (logits.to(DEV), temps.to(DEV), seeds.to(DEV), ctrs.to(DEV))
    out = hip.sample_gumbel(*args).cpu().numpy().astype(np.int64)
    firm = gap >= eo.GUMBEL_GAMMA
    print(f"[elem-oracle] gumbel {B}x{V}: {int((out == best).sum())}/{B} "
          f"rows pick the fp64 best, {int((~firm).sum())} below gamma")
    bad = np.nonzero(firm & (out != best))[0]
    assert bad.size == 0, [(int(r), int(out[r]), int(best[r]), float(gap[r]))
                           for r in bad[:8]]
    assert bool(((out == best) | (out == runner))[~firm].all())
    if B >= 4:
        assert out[0] == out[1], "equal (seed, ctr) rows disagree"
    # greedy rows (T = 0, T = -1): the lowest index of the planted pair
    g = np.nonzero(temps.numpy() <= 0)[0]
    assert (out[g] == logits.float().numpy().argmax(axis=1)[g]).all()
    again = hip.sample_gumbel(*args).cpu().numpy()
    assert (again == out).all()


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("V", eo.REGRESSION_V)
def test_gumbel_noise_is_finite(V, which):
    """One row whose hash has all 24 top bits set at one token (token 5 at
    ctr 0 under the published seed; token V - 1 at ctr 4095 under a solved
    one).  With 24-bit mantissas + 0.5f that is u == 1, g == +inf and the
    token wins against a 30-logit deficit; finite noise cannot."""
    hip = _hip()
    logits, seeds, ctrs = eo.regression_case(V, which)
    temps = torch.ones(3)
    out = hip.sample_gumbel(logits.to(DEV), temps.to(DEV), seeds.to(DEV),
                            ctrs.to(DEV))
    assert out.cpu().tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------
# gumbel, supplied noise


@pytest.mark.parametrize("B", (0, 390))
def test_gumbel_supplied_noise_planted_gap(B):
    """Equal logits, noise 0.5 except 1 - 2^-20 at one index per row (a
    score gap of 13.5): that index must win; with the same value planted
    at a lower index too, the lower one must.  The indices are the argmax
    tie edges plus the first and last Gumbel slice edges; B = 390 repeats
    the rows on the single-block path."""
    hip = _hip()
    V = eo.ARGMAX_V
    seg = (V + 31) // 32
    idx = sorted(set(eo.edge_indices(V)) | {seg - 1, seg, 31 * seg - 1,
                                            31 * seg})
    if B == 0:
        B = len(idx)
        assert 768 // B >= 32                 # 32 slices of `seg`
    else:
        assert 768 // B == 1
    hi = torch.tensor([idx[r % len(idx)] for r in range(B)])
    lo = torch.tensor([idx[max(0, r % len(idx) - 1)] for r in range(B)])
    logits = torch.zeros(B, V, dtype=torch.bfloat16, device=DEV)
    temps = torch.ones(B, device=DEV)
    seeds = torch.zeros(B, dtype=torch.int64, device=DEV)
    ctrs = torch.zeros(B, dtype=torch.int32, device=DEV)
    noise = torch.full((B, V), 0.5)
    noise[torch.arange(B), hi] = 1.0 - 2.0 ** -20
    out = hip.sample_gumbel(logits, temps, seeds, ctrs, noise=noise.to(DEV))
    assert out.cpu().tolist() == hi.tolist()
    noise[torch.arange(B), lo] = 1.0 - 2.0 ** -20
    out = hip.sample_gumbel(logits, temps, seeds, ctrs, noise=noise.to(DEV))
    assert out.cpu().tolist() == lo.tolist()
