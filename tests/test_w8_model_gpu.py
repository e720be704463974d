"""FP8 weight-only models on the GPU, held to the fp64 model oracle
(tests/model_oracle.py) evaluated on the CPU model with the same
quantised weights: live weights bit-equal to the CPU build, packs that
decode to the live weights, prefill, generic decode and fused decode at
MT = 1 and MT = 2 batch sizes within the oracle's budget, fused decode
bit-equal to a bf16 model carrying the same weight values, and an engine
run whose eager, graphed and pipelined tokens agree."""
import dataclasses
import functools

import pytest
import torch

import model_oracle as mo
import test_engine_oracle_gpu as teo
from ollamamq_amd.models import LlamaModel, PRESETS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CONFIGS = {
    "tiny-fp8": PRESETS["tiny-fp8"],
    "qwen-mini-fp8": dataclasses.replace(mo.MINIS["qwen-mini"], quant="fp8"),
}
MATS = ("wqkv", "wo", "wgate_up", "wdown")


@functools.lru_cache(maxsize=None)
def cpu_model(name):
    return LlamaModel(CONFIGS[name], device="cpu", dtype=torch.bfloat16,
                      seed=mo.SEED)


@functools.lru_cache(maxsize=None)
def gpu_model(name):
    from ollamamq_amd.ops import hip
    m = LlamaModel(CONFIGS[name], device=DEV, dtype=torch.bfloat16,
                   seed=mo.SEED)
    assert m.fused_chain, f"{name} should qualify for the fused chain"
    packs = [m.lm_head_pk] + [p for l in m.layers for p in
                              (l.wqkv_pk, l.wo_pk, l.wgu_pk, l.wdown_pk)]
    assert all(isinstance(p, hip.Fp8Pack) for p in packs)
    return m


@functools.lru_cache(maxsize=None)
def bf16_twin(name):
    """A bf16 model whose live weights are overwritten with the fp8
    model's values and repacked: the bf16 kernels over dq(W)."""
    src = gpu_model(name)
    m = LlamaModel(dataclasses.replace(CONFIGS[name], quant=""), device=DEV,
                   dtype=torch.bfloat16, seed=mo.SEED)
    m.lm_head = src.lm_head.clone()
    for a, b in zip(m.layers, src.layers):
        for k in MATS:
            setattr(a, k, getattr(b, k).clone())
    m._pack_weights()
    assert m.fused_chain and torch.is_tensor(m.lm_head_pk)
    return m


@functools.lru_cache(maxsize=None)
def truth_of(name, tag, lens):
    cfg = CONFIGS[name]
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(f"{name}/{tag}"))
    g = torch.Generator().manual_seed(seed)
    seqs = [torch.randint(0, cfg.vocab, (n,), generator=g).tolist()
            for n in lens]
    return (seqs,) + mo.truth_and_budget(cpu_model(name), seqs)


def _rig(model, name, tag, lens, seed=0):
    seqs, truth, budget = truth_of(name, tag, tuple(lens))
    return mo.Rig(model, seqs, DEV, seed), truth, budget.fresh()


def _report(group, name, b):
    lg, kv = b.report()
    print(f"RATIO w8-{group} {name} logits {lg:.3f} kv "
          + " ".join(f"{x:.3f}" for x in kv))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_live_weights_and_packs(name):
    from ollamamq_amd.ops import hip
    g, c = gpu_model(name), cpu_model(name)
    bits = lambda t: t.cpu().view(torch.int16)
    assert torch.equal(bits(g.embed), bits(c.embed))
    assert torch.equal(bits(g.lm_head), bits(c.lm_head))
    V, H = g.lm_head.shape
    assert torch.equal(bits(hip.unpack_weight_fp8(g.lm_head_pk, V, H)),
                       bits(c.lm_head))
    for a, b in zip(g.layers, c.layers):
        for k, pk in zip(MATS, (a.wqkv_pk, a.wo_pk, a.wgu_pk, a.wdown_pk)):
            w = getattr(a, k)
            assert torch.equal(bits(w), bits(getattr(b, k))), k
            assert torch.equal(bits(hip.unpack_weight_fp8(pk, *w.shape)),
                               bits(w)), k
        if b.bqkv is not None:
            assert torch.equal(bits(a.bqkv), bits(b.bqkv))


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_prefill_120(name):
    rig, truth, b = _rig(gpu_model(name), name, "one120", (120,))
    logits, rows = rig.forward([(0, 0, 120)], "prefill", logits_idx=False)
    assert logits.shape[0] == 120
    rig.check(truth, b, logits, rows, "one120")
    _report("prefill", name, b)


def _decode_rig(model, name, B, seed):
    ctx = mo.decode_ctx(B)
    rig, truth, b = _rig(model, name, f"decode{B}", [c + 1 for c in ctx],
                         seed)
    rig.forward([(i, 0, c) for i, c in enumerate(ctx)], "prefill")
    return rig, truth, b, [(i, c, c + 1) for i, c in enumerate(ctx)]


@pytest.mark.parametrize("B", mo.EXACT_B)
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_decode_generic_and_fused(name, B):
    """B = 5 runs MT = 1, B = 40 MT = 2.  The fused logits and pools are
    also bit-equal to the bf16 twin's from the same cache state."""
    rig, truth, b, parts = _decode_rig(gpu_model(name), name, B, seed=B)
    state = rig.save()
    logits, rows = rig.forward(parts, "decode", fused=False)
    rig.check(truth, b, logits, rows, f"B={B} generic")
    _report("generic-decode", name, b)
    b = b.fresh()
    rig.restore(state)
    logits, rows = rig.forward(parts, "decode", fused=True)
    assert logits.shape[0] == B
    rig.check(truth, b, logits, rows, f"B={B} fused")
    _report("fused-MT1" if B <= 32 else "fused-MT2", name, b)
    pools = mo.snapshot(rig.kv)

    twin, _, _, parts2 = _decode_rig(bf16_twin(name), name, B, seed=B)
    assert twin.slots == rig.slots and parts2 == parts
    twin.restore(state)
    l2, _ = twin.forward(parts, "decode", fused=True)
    assert torch.equal(l2, logits), \
        f"fused fp8 logits differ from the bf16 twin's " \
        f"({int((l2 != logits).sum())} elements)"
    p2 = mo.snapshot(twin.kv)
    assert torch.equal(p2[0], pools[0]) and torch.equal(p2[1], pools[1])


def test_engine_three_paths_agree():
    """tiny-fp8, batch 3, 24 greedy tokens each: the same tokens eager,
    graphed and pipelined, every token near the oracle's best under
    teacher forcing."""
    from ollamamq_amd.engine import LlamaEngine, PagedKVCache
    name = "tiny-fp8"
    model = gpu_model(name)
    kv = PagedKVCache.for_model(model.cfg, n_pages=96, max_slots=10,
                                max_ctx=mo.MAX_CTX, device=DEV,
                                dtype=torch.bfloat16)
    mo.scramble(kv, 4)
    eng = LlamaEngine(model, kv, max_batch=8)
    tap = teo.Tap(eng)
    prompts = mo.case_tokens(name, "engine", (10, 58, 30))
    tokens = {}
    for path in ("eager", "graphed", "pipelined"):
        eng.use_graphs = path != "eager"
        eng.use_pipeline = path == "pipelined"
        tap.clear()
        seqs = teo._submit(eng, prompts, [teo._greedy(24)] * 3)
        teo._drive(eng)
        assert all(len(s.generated) == 24 for s in seqs)
        assert (tap.replays == 0) == (path == "eager")
        teo._check(name, tap, seqs, f"{path} w8")
        tokens[path] = [list(s.generated) for s in seqs]
    assert tokens["eager"] == tokens["graphed"] == tokens["pipelined"]
