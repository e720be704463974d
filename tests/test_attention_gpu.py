"""Paged attention kernels vs the fp64 oracle and exact key probes (1 GPU).

k_decode_attn<G,CH> + k_decode_combine (and the in-launch combine),
k_prefill_attn<G>, the legacy VALU k_paged_attn<16> and attention_mixed,
called through ollamamq_amd.ops.hip on adversarial pools
(tests/attn_oracle.py: shuffled slots and pages, a middle layer, NaN in
every row no live (slot, position) owns).  Tier A1 aims each query at one
key and demands that key's V row bit for bit, or the oracle's answer when
the key is invisible; tier A2 counts every visible key exactly once; tier
B holds real-valued outputs to the budgets proven on the CPU in
tests/test_attn_oracle_cpu.py.  The worst normalised error of each tier-B
group is printed so headroom can be recorded (docs/KERNELS.md).
"""
import pytest
import torch

import attn_oracle as ao

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUP_IDS = [f"G{G}-KVH{K}" for G, K in ao.GROUPS]


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


def _report(group, worst):
    print(f"[attn-oracle] {group}: worst normalised error {worst:.3f}")


class _Launch:
    """Sets the decode launch shape the way the wrapper reads it (split and
    fused combine from the environment per call, the chunk from a module
    attribute read at import) and records the split it really used."""

    def __init__(self, hip, monkeypatch):
        self.hip, self.mp, self.splits = hip, monkeypatch, []
        orig = hip._decode_scratch

        def spy(S, Hq, split, dev):
            self.splits.append(split)
            return orig(S, Hq, split, dev)
        monkeypatch.setattr(hip, "_decode_scratch", spy)

    def decode(self, q, pool, meta, chunk, split, fused=False):
        self.mp.setattr(self.hip, "_CHUNK_ENV", str(chunk))
        if split is None:
            self.mp.delenv("OLLAMAMQ_DECODE_SPLIT", raising=False)
        else:
            self.mp.setenv("OLLAMAMQ_DECODE_SPLIT", str(split))
        if fused:
            self.mp.setenv("OLLAMAMQ_FUSED_COMBINE", "1")
        else:
            self.mp.delenv("OLLAMAMQ_FUSED_COMBINE", raising=False)
        want = ao.wrapper_split(q.shape[0], pool.KVH, meta.max_kv, split)
        assert split is None or want == split, (want, split)
        del self.splits[:]
        out = self.hip.attention_decode(q, pool.cache, ao.LAYER, meta)
        assert self.splits == ([want] if want > 1 else []), \
            (self.splits, want)
        return out.cpu()


# ---------------------------------------------------------------------------
# decode


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_decode_probes(G, KVH, monkeypatch):
    """Tier A1 on k_decode_attn: every chunk length and split must return
    the probed key's V row bit for bit; a probe aimed at kv_len or at
    lo_tok - 1 must return the oracle over the visible keys instead."""
    hip = _hip()
    run = _Launch(hip, monkeypatch)
    Hq = G * KVH
    cpu = ao.build_pool(ao.probe_kv(KVH), seed=1, max_ctx=512)
    pool = cpu.to(DEV)
    n_pos = n_neg = 0
    for W in ao.PROBE_DECODE_WINDOWS:
        seqs, lens, targets, positive = ao.decode_probe_plan(Hq, KVH, W)
        S = len(seqs)
        q = ao.probe_queries(seqs, [1] * S, targets, Hq, KVH)
        want = ao.probe_expected(cpu, seqs, [1] * S, targets, Hq)
        truth, _ = ao.oracle_batch(cpu, q, seqs, lens, window=W)
        pos = torch.tensor(positive)
        neg = ~pos
        meta = pool.meta(seqs, lens, window=W, max_kv=512)
        qd = q.to(DEV)
        for chunk in ao.DECODE_CHUNKS:
            for split in ao.DECODE_SPLITS:
                got = run.decode(qd, pool, meta, chunk, split)
                bad = (got[pos] != want[pos]).any(-1)
                assert not bad.any(), \
                    (W, chunk, split, int(bad.sum()), "of", int(pos.sum()))
                assert ao.ratio(got[neg], truth[neg], per_vector=True) \
                    <= 1.0, (W, chunk, split)
                assert not (got[neg] == want[neg]).all(-1).any(), \
                    (W, chunk, split, "an invisible key was returned")
        n_pos += int(pos.sum())
        n_neg += int(neg.sum())
    assert n_pos >= 100 and n_neg >= 20


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_decode_counting(G, KVH, monkeypatch):
    """Tier A2 on k_decode_attn: K = 0, one-hot V; every visible key is
    counted exactly once through every chunk length, split and window."""
    hip = _hip()
    run = _Launch(hip, monkeypatch)
    Hq = G * KVH
    cpu = ao.build_pool(ao.counting_kv(KVH), seed=2)
    pool = cpu.to(DEV)
    for W, lens in [(0, ao.COUNT_DECODE_LENS)] + list(ao.DECODE_WINDOWS):
        S = len(lens)
        seqs = [r % ao.COUNT_SEQS for r in range(S)]
        q = ao.real_q(S, Hq, 1.0, seed=W + 5)
        truth, _ = ao.oracle_batch(cpu, q, seqs, lens, window=W)
        meta = pool.meta(seqs, lens, window=W, max_kv=ao.COUNT_CAP)
        qd = q.to(DEV)
        for chunk in ao.DECODE_CHUNKS:
            for split in ao.DECODE_SPLITS:
                got = run.decode(qd, pool, meta, chunk, split)
                ao.assert_counting(got, truth, f"W{W} CH{chunk} "
                                   f"split {split}")


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_decode_real(G, KVH, monkeypatch):
    """Tier B on k_decode_attn + k_decode_combine: ragged lengths, every
    split (the capture geometry's 32 mostly-empty segments included),
    windows on and past chunk edges, q contiguous (scale 1) and as a
    strided view of a fused qkv buffer (scale 3)."""
    hip = _hip()
    run = _Launch(hip, monkeypatch)
    worst = 0.0
    for gi, (tag, lens, W, splits, max_kv) in enumerate(ao.decode_groups(G)):
        S = len(lens)
        for scale in ao.Q_SCALES:
            kvs, q = ao.decode_inputs(G, KVH, gi, lens, scale)
            cpu = ao.build_pool(kvs, seed=gi, max_ctx=512)
            pool = cpu.to(DEV)
            truth, _ = ao.oracle_batch(cpu, q, range(S), lens, window=W)
            meta = pool.meta(range(S), lens, window=W, max_kv=max_kv)
            qd = q.to(DEV)
            if scale != 1.0:
                qd = ao.strided(qd, KVH)
                assert qd.stride(0) == (G + 2) * KVH * ao.D
            for chunk in ao.DECODE_CHUNKS:
                for split in splits:
                    got = run.decode(qd, pool, meta, chunk, split)
                    if tag == "capture":
                        assert run.splits == [32]
                    worst = max(worst, ao.assert_close(
                        got, truth, [1] * S,
                        what=f"{tag} x{scale} CH{chunk} split {split}"))
                    if W == 1:      # only the last key is visible
                        last = torch.stack([
                            kvs[i][1][n - 1].repeat_interleave(G, dim=0)
                            for i, n in enumerate(lens)])
                        assert torch.equal(got, last)
    _report(f"decode G={G} KVH={KVH}", worst)


@pytest.mark.parametrize("G,KVH", [(4, 2), (7, 2)])
def test_decode_fused_combine(G, KVH, monkeypatch):
    """OLLAMAMQ_FUSED_COMBINE=1 at split 3, twice in a row: the ticket
    counters reset themselves, so the second launch is bit-equal to the
    first and both to the separate k_decode_combine pass."""
    hip = _hip()
    run = _Launch(hip, monkeypatch)
    lens = ao.DECODE_LENS
    S = len(lens)
    kvs, q = ao.decode_inputs(G, KVH, 1, lens, 1.0)
    cpu = ao.build_pool(kvs, seed=1, max_ctx=512)
    pool = cpu.to(DEV)
    truth, _ = ao.oracle_batch(cpu, q, range(S), lens)
    meta = pool.meta(range(S), lens, max_kv=512)
    qd = q.to(DEV)
    for chunk in ao.DECODE_CHUNKS:
        sep = run.decode(qd, pool, meta, chunk, 3)
        one = run.decode(qd, pool, meta, chunk, 3, fused=True)
        two = run.decode(qd, pool, meta, chunk, 3, fused=True)
        ao.assert_close(sep, truth, [1] * S, what=f"separate CH{chunk}")
        assert torch.equal(one, sep) and torch.equal(two, sep)
        sem = hip._combine_sem(S, KVH, qd.device)
        assert int(sem.abs().sum()) == 0


# ---------------------------------------------------------------------------
# prefill


def _prefill(hip, q, pool, meta):
    return hip.attention_prefill(q, pool.cache, ao.LAYER, meta).cpu()


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_prefill_probes(G, KVH):
    """Tier A1 on k_prefill_attn: every query row of a tile carries its own
    target (the diagonal, the window edge, 0, the chunk edges 63/64);
    negative probes aim at p + 1 and p - W."""
    hip = _hip()
    Hq = G * KVH
    cpu = ao.build_pool(ao.probe_kv(KVH), seed=1, max_ctx=512)
    pool = cpu.to(DEV)
    n_neg = 0
    for W in ao.PROBE_PREFILL_WINDOWS:
        cases = ao.PREFILL_WINDOW_CASES if W else ao.PREFILL_CASES
        seqs, lens, qls, targets, positive = ao.prefill_probe_plan(
            Hq, cases, W)
        q = ao.probe_queries(seqs, qls, targets, Hq, KVH)
        want = ao.probe_expected(cpu, seqs, qls, targets, Hq)
        truth, absp = ao.oracle_batch(cpu, q, seqs, lens, qls, W)
        pos = torch.tensor(positive)
        neg = ~pos
        got = _prefill(hip, q.to(DEV), pool, pool.meta(seqs, lens, qls, W))
        bad = (got[pos] != want[pos]).any(-1)
        assert not bad.any(), (W, int(bad.sum()), "of", int(pos.sum()))
        assert ao.ratio(got[neg], truth[neg], absp[neg], per_vector=True) \
            <= 1.0, W
        assert not (got[neg] == want[neg]).all(-1).any(), \
            (W, "an invisible key was returned")
        n_neg += int(neg.sum())
    assert n_neg >= 50


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_prefill_counting(G, KVH):
    """Tier A2 on k_prefill_attn (P = 1 is exact in bf16, so the decode
    budget applies) for every window."""
    hip = _hip()
    Hq = G * KVH
    cpu = ao.build_pool(ao.counting_kv(KVH), seed=2)
    pool = cpu.to(DEV)
    for W, cases in ao.prefill_runs():
        qls = [a for a, _ in cases]
        lens = [b for _, b in cases]
        seqs = [i % ao.COUNT_SEQS for i in range(len(cases))]
        q = ao.real_q(sum(qls), Hq, 1.0, seed=W + 3)
        truth, _ = ao.oracle_batch(cpu, q, seqs, lens, qls, W)
        got = _prefill(hip, q.to(DEV), pool, pool.meta(seqs, lens, qls, W))
        ao.assert_counting(got, truth, f"W{W}")


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_prefill_real(G, KVH):
    """Tier B on k_prefill_attn: whole, ragged and continued chunks, every
    window, q contiguous (scale 1) and strided (scale 3)."""
    hip = _hip()
    worst = 0.0
    for wi, (W, cases) in enumerate(ao.prefill_runs()):
        qls = [a for a, _ in cases]
        lens = [b for _, b in cases]
        n = len(cases)
        for scale in ao.Q_SCALES:
            kvs, q = ao.prefill_inputs(G, KVH, wi, cases, scale)
            cpu = ao.build_pool(kvs, seed=20 + wi)
            pool = cpu.to(DEV)
            truth, absp = ao.oracle_batch(cpu, q, range(n), lens, qls, W)
            qd = q.to(DEV)
            if scale != 1.0:
                qd = ao.strided(qd, KVH)
            got = _prefill(hip, qd, pool, pool.meta(range(n), lens, qls, W))
            worst = max(worst, ao.assert_close(got, truth, qls, absp,
                                               what=f"W{W} x{scale}"))
            if W == 1:
                last = torch.cat([
                    kvs[i][1][b - a:b].repeat_interleave(G, dim=1)
                    for i, (a, b) in enumerate(cases)])
                assert torch.equal(got, last)
    _report(f"prefill G={G} KVH={KVH}", worst)


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_prefill_valu_fallback(G, KVH, monkeypatch):
    """OLLAMAMQ_VALU_PREFILL=1 runs the legacy k_paged_attn<16>; it keeps
    p in fp32, so it is held to the decode budget."""
    hip = _hip()
    monkeypatch.setenv("OLLAMAMQ_VALU_PREFILL", "1")
    cases = ao.PREFILL_CASES
    qls = [a for a, _ in cases]
    lens = [b for _, b in cases]
    n = len(cases)
    worst = 0.0
    for scale in ao.Q_SCALES:
        kvs, q = ao.prefill_inputs(G, KVH, 0, cases, scale)
        cpu = ao.build_pool(kvs, seed=20)
        pool = cpu.to(DEV)
        truth, _ = ao.oracle_batch(cpu, q, range(n), lens, qls)
        qd = q.to(DEV)
        if scale != 1.0:
            qd = ao.strided(qd, KVH)
        meta = pool.meta(range(n), lens, qls)
        got = _prefill(hip, qd, pool, meta)
        assert hasattr(meta, "_plan_16") and \
            not hasattr(meta, f"_plan_{hip.PREFILL_QT}")
        worst = max(worst, ao.assert_close(got, truth, qls,
                                           what=f"valu x{scale}"))
    _report(f"valu prefill G={G} KVH={KVH}", worst)


# ---------------------------------------------------------------------------
# mixed


@pytest.mark.parametrize("window", ao.MIXED_WINDOWS)
@pytest.mark.parametrize("G,KVH", [(4, 2), (7, 2)])
def test_mixed(G, KVH, window):
    """attention_mixed: three decode rows, then a fresh and a continued
    prefill chunk.  Held to the oracle and bit-equal to the separate
    attention_decode / attention_prefill results on the same rows."""
    hip = _hip()
    nd = len(ao.MIXED_DECODE_LENS)
    lens = list(ao.MIXED_DECODE_LENS) + [b for _, b in ao.MIXED_PREFILL]
    qls = [1] * nd + [a for a, _ in ao.MIXED_PREFILL]
    n = len(lens)
    worst = 0.0
    for scale in ao.Q_SCALES:
        seed = ao.case_seed(G, KVH, 40)
        kvs = ao.real_kv(lens, KVH, seed)
        q = ao.real_q(sum(qls), G * KVH, scale, seed + int(scale))
        cpu = ao.build_pool(kvs, seed=40)
        pool = cpu.to(DEV)
        truth, absp = ao.oracle_batch(cpu, q, range(n), lens, qls, window)
        qd = q.to(DEV)
        meta = pool.meta(range(n), lens, qls, window, mode="mixed",
                         n_decode=nd)
        got = hip.attention_mixed(qd, pool.cache, ao.LAYER, meta).cpu()
        worst = max(worst, ao.assert_close(
            got[:nd], truth[:nd], [1] * nd, what=f"decode rows x{scale}"))
        worst = max(worst, ao.assert_close(
            got[nd:], truth[nd:], qls[nd:], absp[nd:],
            what=f"prefill rows x{scale}"))
        dec = hip.attention_decode(
            qd[:nd], pool.cache, ao.LAYER,
            pool.meta(range(nd), lens[:nd], window=window,
                      max_kv=meta.max_kv)).cpu()
        pre = hip.attention_prefill(
            qd[nd:], pool.cache, ao.LAYER,
            pool.meta(range(nd, n), lens[nd:], qls[nd:], window)).cpu()
        assert torch.equal(got[:nd], dec)
        assert torch.equal(got[nd:], pre)
    _report(f"mixed G={G} KVH={KVH} W={window}", worst)
