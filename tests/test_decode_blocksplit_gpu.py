"""k_decode_attn_blk (decode attention with all KV segments of a (sequence,
kv-head) in one block, merged through LDS) against the two-kernel split
path it replaces and against the fp64 oracle (1 GPU).

Pools, oracle, budgets and the exact tiers are those of tests/attn_oracle.py
(shuffled non-ascending pages, a shuffled slot subset, NaN in every unowned
row, the middle of three layers).  Every run is made twice through the
block path and once through OLLAMAMQ_DECODE_BLOCKSPLIT=0 at the same forced
split, in the standard and the frag output layout: the three must be
bit-equal, free of NaN and inside the decode tier-B budget.
"""
import pytest
import torch

import attn_oracle as ao
import fused_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# fewer chunks than segments, exactly NSEG chunks, uneven 2/2/2/3 bounds
RAGGED = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200, 257)
# (G, KVH, split): every instantiated head count class at split 4, the
# 8- and 16-wave blocks at split 2, and a KVH that is no power of two
GROUPS = [(1, 2, 4), (2, 2, 4), (4, 2, 4), (4, 2, 2), (8, 2, 2), (3, 3, 4)]


class _Run:
    """attention_decode at a forced split through either path; checks which
    path ran by whether it asked for partial scratch."""

    def __init__(self, monkeypatch):
        from ollamamq_amd.ops import hip
        hip.require()
        self.hip, self.mp, self.scratch = hip, monkeypatch, []
        orig = hip._decode_scratch

        def spy(S, Hq, split, dev):
            self.scratch.append(split)
            return orig(S, Hq, split, dev)
        monkeypatch.setattr(hip, "_decode_scratch", spy)
        monkeypatch.setattr(hip, "_CHUNK_ENV", None)
        monkeypatch.delenv("OLLAMAMQ_FUSED_COMBINE", raising=False)

    def __call__(self, q, pool, meta, split, blk, fragout=False):
        S, Hq, _ = q.shape
        self.mp.setenv("OLLAMAMQ_DECODE_SPLIT", str(split))
        self.mp.setenv("OLLAMAMQ_DECODE_BLOCKSPLIT", "1" if blk else "0")
        assert ao.wrapper_split(S, pool.KVH, meta.max_kv, split) == split
        del self.scratch[:]
        out = self.hip.attention_decode(q, pool.cache, ao.LAYER, meta,
                                        fragout=fragout)
        assert self.scratch == ([] if blk else [split]), \
            ("wrong path", blk, self.scratch)
        if fragout:
            out = fo.from_frag(out, S, Hq * ao.D).reshape(S, Hq, ao.D)
        return out.cpu()

    def both(self, q, pool, meta, split, what):
        """The block path's output after the equalities that every case
        asserts."""
        ref = self(q, pool, meta, split, blk=False)
        for fragout in (False, True):
            old = ref if not fragout else \
                self(q, pool, meta, split, blk=False, fragout=True)
            one = self(q, pool, meta, split, blk=True, fragout=fragout)
            two = self(q, pool, meta, split, blk=True, fragout=fragout)
            tag = f"{what} split {split} fragout {fragout}"
            assert not torch.isnan(one.float()).any(), tag
            assert torch.equal(one, old), f"{tag}: differs from two-kernel"
            assert torch.equal(two, one), f"{tag}: second call differs"
            assert torch.equal(old, ref), f"{tag}: layouts disagree"
        return one


def _real_case(run, G, KVH, lens, splits, window=0, max_kv=512, seed=0,
               max_ctx=512, what=""):
    S = len(lens)
    kvs, q = ao.decode_inputs(G, KVH, 50 + seed, lens, 1.0)
    cpu = ao.build_pool(kvs, seed=seed, max_ctx=max_ctx)
    pool = cpu.to(DEV)
    truth, _ = ao.oracle_batch(cpu, q, range(S), lens, window=window)
    meta = pool.meta(range(S), lens, window=window, max_kv=max_kv)
    qd = q.to(DEV)
    worst = 0.0
    for split in splits:
        got = run.both(qd, pool, meta, split, what)
        worst = max(worst, ao.assert_close(got, truth, [1] * S,
                                           what=f"{what} split {split}"))
        if window == 1:             # only the last key is visible
            last = torch.stack([kvs[i][1][n - 1].repeat_interleave(G, dim=0)
                                for i, n in enumerate(lens)])
            assert torch.equal(got, last)
    print(f"[blocksplit] {what} G={G} KVH={KVH}: worst normalised error "
          f"{worst:.3f}")


@pytest.mark.parametrize("G,KVH,split", GROUPS,
                         ids=[f"G{g}-KVH{k}-split{s}" for g, k, s in GROUPS])
def test_ragged(G, KVH, split, monkeypatch):
    """Ragged batch, every instantiated block shape."""
    _real_case(_Run(monkeypatch), G, KVH, RAGGED, (split,), seed=split,
               what="ragged")


def test_s33(monkeypatch):
    """33 sequences: the last one lands in the second 32-row frag half."""
    _real_case(_Run(monkeypatch), 4, 2, ao.S33_LENS, (4,), seed=3,
               what="S33")


def test_capture_geometry(monkeypatch):
    """max_kv = the pool's max_ctx with short sequences: most segments are
    empty, and with one active chunk only segment NSEG-1 has work."""
    for split in (2, 4):
        assert ao.decode_segments(1, 0, 64, split)[1][:-1] == \
            [(0, 0)] * (split - 1)
    _real_case(_Run(monkeypatch), 4, 2, ao.CAPTURE_LENS, (2, 4),
               max_kv=ao.CAPTURE_MAX_KV, max_ctx=ao.CAPTURE_MAX_KV, seed=4,
               what="capture")


@pytest.mark.parametrize("W,lens", ao.DECODE_WINDOWS,
                         ids=[f"W{w}" for w, _ in ao.DECODE_WINDOWS])
def test_windows(W, lens, monkeypatch):
    """Sliding windows with lo_tok on and just past a chunk edge."""
    _real_case(_Run(monkeypatch), 4, 2, lens, (2, 4), window=W, seed=5 + W,
               what=f"W{W}")


def _probe_plan(Hq, window, CH):
    """Rows aimed at every segment's first and last key under splits 2 and
    4, at kv_len - 1 and at lo_tok; one target per head."""
    lens = (1, 17, 64, 65, 129, 200, 257, 300) if window == 0 \
        else (40, 100, 101, 164, 165, 300)
    seqs, kv_lens, targets = [], [], []
    for n in lens:
        lo = n - window if (window > 0 and n > window) else 0
        pos = {n - 1, lo}
        for split in (2, 4):
            for c0, c1 in ao.decode_segments(n, window, CH, split)[1]:
                if c0 < c1:
                    pos.add(max(c0 * CH, lo))
                    pos.add(min(c1 * CH, n) - 1)
        pos = sorted(pos)
        assert all(lo <= t < n for t in pos)
        pos += (pos * Hq)[:-len(pos) % Hq]  # whole rows: repeat from the start
        for r in range(0, len(pos), Hq):
            seqs.append(len(seqs) % ao.PROBE_SEQS)
            kv_lens.append(n)
            targets.append(pos[r:r + Hq])
    return seqs, kv_lens, targets


@pytest.mark.parametrize("G,KVH", [(4, 2), (1, 2)], ids=["G4", "G1"])
def test_probes(G, KVH, monkeypatch):
    """Tier A1 through the block path: the softmax is exactly one-hot, so
    each head must return its target key's V row bit for bit."""
    run = _Run(monkeypatch)
    Hq = G * KVH
    cpu = ao.build_pool(ao.probe_kv(KVH), seed=1, max_ctx=512)
    pool = cpu.to(DEV)
    n = 0
    for W in (0, 100):
        seqs, lens, targets = _probe_plan(Hq, W, run.hip._decode_chunk(G))
        S = len(seqs)
        q = ao.probe_queries(seqs, [1] * S, targets, Hq, KVH).to(DEV)
        want = ao.probe_expected(cpu, seqs, [1] * S, targets, Hq)
        meta = pool.meta(seqs, lens, window=W, max_kv=512)
        for split in (2, 4):
            got = run.both(q, pool, meta, split, f"probes W{W}")
            bad = (got != want).any(-1)
            assert not bad.any(), (W, split, int(bad.sum()), "of", S * Hq)
        n += S * Hq
    assert n >= 80


def test_counting(monkeypatch):
    """Tier A2 through the block path: K = 0, one-hot V; every visible key
    is counted exactly once."""
    run = _Run(monkeypatch)
    G, KVH = 4, 2
    cpu = ao.build_pool(ao.counting_kv(KVH), seed=2)
    pool = cpu.to(DEV)
    for W, lens in [(0, ao.COUNT_DECODE_LENS)] + list(ao.DECODE_WINDOWS):
        S = len(lens)
        seqs = [r % ao.COUNT_SEQS for r in range(S)]
        q = ao.real_q(S, G * KVH, 1.0, seed=W + 5)
        truth, _ = ao.oracle_batch(cpu, q, seqs, lens, window=W)
        meta = pool.meta(seqs, lens, window=W, max_kv=ao.COUNT_CAP)
        for split in (2, 4):
            got = run.both(q.to(DEV), pool, meta, split, f"counting W{W}")
            ao.assert_counting(got, truth, f"W{W} split {split}")


def test_graph_replays(monkeypatch):
    """The op captured with seq_lens advanced by a trailing add: three
    replays are bit-equal to three eager calls on the same lengths."""
    run = _Run(monkeypatch)
    G, KVH, split, steps = 4, 2, 4, 3
    lens = [n for n in RAGGED]
    S = len(lens)
    # each sequence owns `steps` rows more than its starting length
    kvs, q = ao.decode_inputs(G, KVH, 60, [n + steps for n in lens], 1.0)
    cpu = ao.build_pool(kvs, seed=6, max_ctx=512)
    pool = cpu.to(DEV)
    meta = pool.meta(range(S), lens, max_kv=512)
    lens0 = meta.seq_lens.clone()
    qd = q.to(DEV)
    monkeypatch.setenv("OLLAMAMQ_DECODE_SPLIT", str(split))
    monkeypatch.setenv("OLLAMAMQ_DECODE_BLOCKSPLIT", "1")

    def step():
        out = run.hip.attention_decode(qd, pool.cache, ao.LAYER, meta)
        meta.seq_lens.add_(1)
        return out

    eager = [step().clone() for _ in range(steps)]
    assert run.scratch == []
    for k, e in enumerate(eager):
        truth, _ = ao.oracle_batch(cpu, q, range(S), [n + k for n in lens])
        ao.assert_close(e, truth, [1] * S, what=f"eager step {k}")
    meta.seq_lens.copy_(lens0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    assert torch.equal(meta.seq_lens, lens0)         # capture runs nothing
    for k in range(steps):
        g.replay()
        assert torch.equal(out, eager[k]), f"replay {k} differs from eager"
    assert torch.equal(meta.seq_lens, lens0 + steps)
    assert run.scratch == []
