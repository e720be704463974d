"""LlamaModel.forward held to the fp64 model oracle (tests/model_oracle.py),
called directly, no engine: prefill (one long prompt, varlen with
logits_idx, continued chunks), decode through the generic path and through
the fused chain at MT=1 and MT=2 batch sizes with the eager and the
capture attention geometry, and mixed batches.  Every case runs on a
scrambled cache (shuffled slots and pages, pattern-filled pools) and
checks the logits rows, every live K/V row of every layer, and that
nothing outside the owned rows changed.  Two exact claims on the fused
chain: scratch contents do not matter, and batch rows do not interact."""
import functools

import pytest
import torch

import model_oracle as mo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def gpu_model(name):
    from ollamamq_amd.models import LlamaModel
    m = LlamaModel(mo.config(name), device=DEV, dtype=torch.bfloat16,
                   seed=mo.SEED)
    assert m.fused_chain, f"{name} should qualify for the fused chain"
    return m


def _rig(name, tag, lens, seed=0):
    seqs, truth, budget = mo.truth_of(name, tag, tuple(lens))
    return mo.Rig(gpu_model(name), seqs, DEV, seed), truth, budget.fresh()


def _report(group, name, b):
    lg, kv = b.report()
    print(f"RATIO {group} {name} logits {lg:.3f} kv "
          + " ".join(f"{x:.3f}" for x in kv))


# ---------------------------------------------------------------------------
# prefill


@pytest.mark.parametrize("name", mo.CONFIGS)
def test_prefill_one_sequence_all_rows(name):
    """120 tokens (past tiny-swa's window), logits_idx=None: every
    position's logits row is checked."""
    rig, truth, b = _rig(name, *mo.PREFILL_CASES[0])
    logits, rows = rig.forward([(0, 0, 120)], "prefill", logits_idx=False)
    assert logits.shape[0] == 120
    rig.check(truth, b, logits, rows, "one120")
    _report("prefill", name, b)


@pytest.mark.parametrize("name", mo.CONFIGS)
def test_prefill_varlen_logits_idx(name):
    tag, lens = mo.PREFILL_CASES[1]
    rig, truth, b = _rig(name, tag, lens, seed=1)
    logits, rows = rig.forward([(i, 0, n) for i, n in enumerate(lens)],
                               "prefill")
    assert logits.shape[0] == len(lens)
    rig.check(truth, b, logits, rows, "varlen")
    _report("prefill", name, b)


@pytest.mark.parametrize("name", mo.CONFIGS)
def test_prefill_continued_chunks(name):
    """A prompt in chunks of 16 and 23."""
    rig, truth, b = _rig(name, *mo.PREFILL_CASES[2], seed=2)
    logits, rows = rig.forward([(0, 0, 16)], "prefill")
    rig.check(truth, b, logits, rows, "chunk 1")
    logits, rows = rig.forward([(0, 16, 39)], "prefill", logits_idx=False)
    assert logits.shape[0] == 23
    rig.check(truth, b, logits, rows, "chunk 2")
    _report("prefill", name, b)


# ---------------------------------------------------------------------------
# decode


def _decode_rig(name, B, seed):
    """Contexts prefilled through the generic path in one varlen forward;
    returns the rig ready for the decode step and its saved state."""
    ctx = mo.decode_ctx(B)
    rig, truth, b = _rig(name, f"decode{B}", [c + 1 for c in ctx], seed)
    rig.forward([(i, 0, c) for i, c in enumerate(ctx)], "prefill")
    return rig, truth, b, [(i, c, c + 1) for i, c in enumerate(ctx)]


@pytest.mark.parametrize("fused", (False, True), ids=("generic", "fused"))
@pytest.mark.parametrize("B", mo.DECODE_B)
@pytest.mark.parametrize("name", mo.CONFIGS)
def test_decode(name, B, fused):
    """One decode step over ragged contexts (1, 15, 16, 17, 63, 64, 65,
    ...), with the eager meta and with the capture geometry
    (max_kv = kv.max_ctx)."""
    rig, truth, b, parts = _decode_rig(name, B, seed=B)
    state = rig.save()
    for capture in (False, True):
        rig.restore(state)
        logits, rows = rig.forward(parts, "decode", fused=fused,
                                   capture=capture)
        assert logits.shape[0] == B
        rig.check(truth, b, logits, rows,
                  f"B={B} fused={fused} capture={capture}")
    group = "generic-decode" if not fused else \
        ("fused-MT1" if B <= 32 else "fused-MT2")
    _report(group, name, b)


# ---------------------------------------------------------------------------
# mixed


@pytest.mark.parametrize("name", mo.CONFIGS)
def test_mixed(name):
    """Three decode rows, a fresh chunk and a continued chunk (88 + 12) in
    one forward; on tiny-swa two decode rows and the continued chunk are
    past the window."""
    lens = mo.MIXED_LENS
    rig, truth, b = _rig(name, "mixed", lens, seed=3)
    rig.forward([(0, 0, lens[0] - 1), (1, 0, lens[1] - 1),
                 (2, 0, lens[2] - 1), (4, 0, mo.MIXED_CONT)], "prefill")
    logits, rows = rig.forward(
        [(0, lens[0] - 1, lens[0]), (1, lens[1] - 1, lens[1]),
         (2, lens[2] - 1, lens[2]), (3, 0, lens[3]),
         (4, mo.MIXED_CONT, lens[4])], "mixed")
    assert logits.shape[0] == 5
    rig.check(truth, b, logits, rows, "mixed")
    _report("mixed", name, b)


# ---------------------------------------------------------------------------
# exact tier


@pytest.mark.parametrize("B", mo.EXACT_B)
@pytest.mark.parametrize("name", ("tiny", "qwen-mini"))
def test_fused_scratch_poison_invariance(name, B):
    """_res_frag, _sq_a and _sq_b are pure scratch: NaN-filled or
    zero-filled before the forward, logits and pools are bit-equal."""
    rig, truth, b, parts = _decode_rig(name, B, seed=10 + B)
    state = rig.save()
    m = rig.model
    out = []
    for fill in (0.0, float("nan")):
        rig.restore(state)
        for t in (m._res_frag, m._sq_a, m._sq_b):
            t.fill_(fill)
        logits, rows = rig.forward(parts, "decode", fused=True)
        rig.check(truth, b, logits, rows, f"fill {fill}")
        out.append((logits.clone(), mo.snapshot(rig.kv)))
    assert torch.equal(out[0][0], out[1][0]), "logits depend on scratch"
    assert torch.equal(out[0][1][0], out[1][1][0]), "k_pool depends on scratch"
    assert torch.equal(out[0][1][1], out[1][1][1]), "v_pool depends on scratch"


@pytest.mark.parametrize("B", mo.EXACT_B)
@pytest.mark.parametrize("name", ("tiny", "qwen-mini"))
def test_fused_row_permutation(name, B):
    """Permuting the batch rows (tok, pos, slot, lens) at the same max_kv
    permutes the logits rows bit for bit and leaves identical pools; at
    B = 40 rows cross the 32-row frag boundary."""
    rig, truth, b, parts = _decode_rig(name, B, seed=20 + B)
    state = rig.save()
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(B)) \
        .tolist()
    if B > 32:
        assert any((i < 32) != (p < 32) for i, p in enumerate(perm))
    la, rows = rig.forward(parts, "decode", fused=True)
    rig.check(truth, b, la, rows, "identity order")
    pa = mo.snapshot(rig.kv)
    rig.restore(state)
    lb, rows = rig.forward(parts, "decode", fused=True, order=perm)
    rig.check(truth, b, lb, rows, "permuted order")
    pb = mo.snapshot(rig.kv)
    assert torch.equal(lb, la[torch.tensor(perm, device=la.device)]), \
        "a row's logits depend on its index in the batch"
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]), \
        "a row's K/V depend on its index in the batch"
