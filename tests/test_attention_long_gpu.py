"""Paged attention kernels vs the fp64 oracle at serving-length contexts
(1 GPU): sequences of up to 8192 keys, so a slot uses up to 513 page-table
entries, a decode segment sweeps up to 256 chunks, a prefill plan has up to
33 query tiles per sequence, continued chunks start thousands of keys in
and sliding windows are 1024 and 4096 keys wide.

Pools, oracle and budgets are those of tests/attn_oracle.py (shuffled
non-ascending pages, a shuffled slot subset, the middle of three layers, NaN
in every unowned row and behind every unowned page-table entry); the long
case lists live there too, and tests/test_attn_long_oracle_cpu.py proves the
yardsticks on the CPU at the same shapes.  Three tiers, as in
tests/test_attention_gpu.py:
  counting  K = 0, one-hot V in two patterns that together give a key's
            position modulo 16384: the output is an exact count ratio;
  probes    K = 0 except 32 x (+-1 code) target keys, q = the code: the
            softmax is one-hot in fp32 and the output is V[t] bit for bit;
  real      N(0,1) inputs against the project's two budgets, on bf16 pools
            and on an fp8 pool next to its bf16 twin.
The worst normalised error of each real-valued group is printed
(docs/KERNELS.md records them).  One model-level case (test_model_long,
tests/model_oracle.py) runs RoPE, append and attention together on a
2100-token prompt.
"""
import pytest
import torch

import attn_oracle as ao
import model_oracle as mo
from ollamamq_amd.engine import PagedKVCache
from ollamamq_amd.ops import quant

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GROUP_IDS = [f"G{G}-KVH{K}" for G, K in ao.LONG_GROUPS]
# more slots than any batch here has rows
SLOTS = 256


def _report(group, worst):
    print(f"[attn-long] {group}: worst normalised error {worst:.3f}")


class _Run:
    """attention_decode at the wrapper's own chunk with the split and the
    block-split gate set through the environment; checks which kernel ran
    by whether the wrapper asked for partial scratch, and records it."""

    def __init__(self, monkeypatch):
        from ollamamq_amd.ops import hip
        hip.require()
        self.hip, self.mp, self.scratch, self.paths = hip, monkeypatch, [], \
            set()
        orig = hip._decode_scratch

        def spy(S, Hq, split, dev):
            self.scratch.append(split)
            return orig(S, Hq, split, dev)
        monkeypatch.setattr(hip, "_decode_scratch", spy)
        monkeypatch.setattr(hip, "_CHUNK_ENV", None)
        monkeypatch.delenv("OLLAMAMQ_FUSED_COMBINE", raising=False)

    def decode(self, q, pool, meta, split, blk):
        """split None = the wrapper's choice; blk None / "0" / "1" is
        OLLAMAMQ_DECODE_BLOCKSPLIT."""
        S, Hq, _ = q.shape
        KVH = pool.KVH
        G = Hq // KVH
        for var, val in (("OLLAMAMQ_DECODE_SPLIT", split),
                         ("OLLAMAMQ_DECODE_BLOCKSPLIT", blk)):
            if val is None:
                self.mp.delenv(var, raising=False)
            else:
                self.mp.setenv(var, str(val))
        want = ao.wrapper_split(S, KVH, meta.max_kv, split)
        assert split is None or want == split, (want, split)
        chunk = self.hip._decode_chunk(G)
        on_blk = self.hip.decode_blocksplit(S, KVH, G, chunk, want)
        del self.scratch[:]
        out = self.hip.attention_decode(q, pool.cache, ao.LAYER, meta)
        assert self.scratch == ([] if on_blk or want == 1 else [want]), \
            ("wrong path", on_blk, want, self.scratch)
        self.paths.add((chunk, want, on_blk))
        return out.cpu()

    def sweep(self, q, pool, meta, splits=ao.LONG_SPLITS):
        """(tag, output) at every split through both gate settings."""
        for split in splits:
            for blk in ("0", "1"):
                yield (f"split {split} blk {blk}",
                       self.decode(q, pool, meta, split, blk))


def _blk_split(G):
    return 4 if G <= 4 else 2


def _prefill(q, pool, meta):
    from ollamamq_amd.ops import hip
    hip.require()
    out = hip.attention_prefill(q, pool.cache, ao.LAYER, meta).cpu()
    # tiles the wrapper planned for its longest sequence
    tile_slot = getattr(meta, f"_plan_{hip.PREFILL_QT}")[0]
    return out, int(torch.bincount(tile_slot.cpu()).max())


# ---------------------------------------------------------------------------
# counting tier


@pytest.mark.parametrize("pattern", [0, 1], ids=["mod128", "div128"])
@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_decode_counting(G, KVH, pattern, monkeypatch):
    """Ragged lengths 511..8192 in one batch on a max_ctx = 8192 cache:
    every split with both gate settings (k_decode_attn + combine and
    k_decode_attn_blk<., ., 2 / 4> with full segments), the capture geometry
    and a batch large enough for the wrapper to pick the block path."""
    run = _Run(monkeypatch)
    Hq = G * KVH
    lens = ao.LONG_DECODE_LENS
    S = len(lens)
    cpu = ao.build_pool(ao.counting_kv_long(lens, KVH, pattern),
                        seed=30 + pattern, max_ctx=ao.LONG_CTX,
                        max_slots=SLOTS)
    pool = cpu.to(DEV)
    q = ao.real_q(S, Hq, 1.0, seed=31)
    truth, _ = ao.oracle_batch(cpu, q, range(S), lens)
    meta = pool.meta(range(S), lens, max_kv=ao.LONG_CTX)
    for tag, got in run.sweep(q.to(DEV), pool, meta):
        ao.assert_counting_long(got, truth, f"ragged {tag}")
    # both block-split instantiations ran unless G allows only one
    blk = {s for _, s, on in run.paths if on}
    assert blk == ({2, 4} if G <= 4 else {2}), run.paths
    assert {s for _, s, on in run.paths if not on} >= {1, 8, 32}

    # the capture geometry proper: 1 and 70 keys beside 4096 and 8192
    seqs = [0, 1, lens.index(4096), lens.index(8192)]
    clens = ao.LONG_CAPTURE_LENS
    qc = ao.real_q(len(seqs), Hq, 1.0, seed=32)
    truth, _ = ao.oracle_batch(cpu, qc, seqs, clens)
    meta = pool.meta(seqs, clens, max_kv=cpu.cache.max_ctx)
    assert ao.wrapper_split(len(seqs), KVH, meta.max_kv) == 32
    for blk in (None, "0"):
        got = run.decode(qc.to(DEV), pool, meta, None, blk)
        ao.assert_counting_long(got, truth, f"capture blk {blk}")

    # 128 rows at max_kv = 4096: the wrapper's own split and gate.  K = 0,
    # so the truth of a row is that of its sequence whatever its query.
    short = [i for i, n in enumerate(lens) if n <= 4096]
    rows = [short[r % len(short)] for r in range(128)]
    rlens = [lens[i] for i in rows]
    qr = ao.real_q(128, Hq, 1.0, seed=33)
    t10, _ = ao.oracle_batch(cpu, qr[:len(short)], short,
                             [lens[i] for i in short])
    truth = t10[[r % len(short) for r in range(128)]]
    meta = pool.meta(rows, rlens, max_kv=4096)
    run.paths.clear()
    got = run.decode(qr.to(DEV), pool, meta, None, None)
    ao.assert_counting_long(got, truth, "128 rows")
    chunk, split, on_blk = next(iter(run.paths))
    if KVH == 2:            # S * KVH = 256: k_decode_attn_blk<G, chunk, 4>
        assert (split, on_blk) == (4, True), run.paths
        assert max(ao.decode_segments(4096, 0, chunk, 4)[1][0]) \
            == 4096 // chunk // 4


@pytest.mark.parametrize("W", ao.LONG_WINDOWS)
@pytest.mark.parametrize("pattern", [0, 1], ids=["mod128", "div128"])
@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_decode_counting_window(G, KVH, pattern, W, monkeypatch):
    """Windows of 1024 and 4096 keys with lo_tok on a chunk edge and just
    past one, far from position 0."""
    run = _Run(monkeypatch)
    lens = ao.long_window_lens(W)
    S = len(lens)
    cpu = ao.build_pool(ao.counting_kv_long(lens, KVH, pattern),
                        seed=40 + pattern, max_ctx=ao.LONG_WINDOW_CTX,
                        max_slots=SLOTS)
    pool = cpu.to(DEV)
    q = ao.real_q(S, G * KVH, 1.0, seed=41)
    truth, _ = ao.oracle_batch(cpu, q, range(S), lens, window=W)
    meta = pool.meta(range(S), lens, window=W, max_kv=ao.LONG_WINDOW_CTX)
    for tag, got in run.sweep(q.to(DEV), pool, meta):
        ao.assert_counting_long(got, truth, f"W{W} {tag}")


@pytest.mark.parametrize("pattern", [0, 1], ids=["mod128", "div128"])
@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_prefill_counting(G, KVH, pattern):
    """Fresh chunks of up to 33 tiles, continued chunks that start 3584,
    4064 and 8191 keys in, and both windows on a chunk of 300 rows that
    crosses the window edge of a 4200-key sequence."""
    cases = ao.LONG_PREFILL_FRESH + ao.LONG_PREFILL_CONT
    wq, wn = ao.LONG_PREFILL_WINDOW_CASE
    lens = [b for _, b in cases] + [wn]
    cpu = ao.build_pool(ao.counting_kv_long(lens, KVH, pattern),
                        seed=50 + pattern, max_ctx=ao.LONG_CTX)
    pool = cpu.to(DEV)
    Hq = G * KVH
    runs = [(0, list(range(len(cases))), [a for a, _ in cases], lens[:-1])]
    runs += [(W, [len(cases)], [wq], [wn]) for W in ao.LONG_WINDOWS]
    for W, seqs, qls, kls in runs:
        q = ao.real_q(sum(qls), Hq, 1.0, seed=51 + W)
        truth, _ = ao.oracle_batch(cpu, q, seqs, kls, qls, W)
        got, tiles = _prefill(q.to(DEV), pool, pool.meta(seqs, kls, qls, W))
        assert tiles == (33 if W == 0 else 10)
        ao.assert_counting_long(got, truth, f"W{W}")


# ---------------------------------------------------------------------------
# single-target probes


def _probe_decode_pool(G, KVH):
    """Positive sequence i and negative sequence len(cases) + i of decode
    probe case i; (cpu pool, cases, targets per case)."""
    CH = 32 if G == 1 else 64
    cases = ao.long_decode_probe_cases()
    kvs, targets = [], []
    for i, (n, W) in enumerate(cases):
        tg = ao.long_probe_targets(n, W, CH, (2, 4, 8, 32))
        targets.append(tg)
        kvs.append(ao.long_probe_kv(n, KVH, tg, seed=600 + i))
    for i, (n, W) in enumerate(cases):
        lo = n - W if (W > 0 and n > W) else 0
        neg = [t for t in (n, lo - 1) if t >= 0]
        K, V = ao.long_probe_kv(n + 1, KVH, [], seed=620 + i)
        K[torch.tensor(neg)] = (32 * ao.probe_codes()[0]).bfloat16()
        kvs.append((K, V))
    return ao.build_pool(kvs, seed=60 + G, max_ctx=ao.LONG_WINDOW_CTX,
                         max_slots=SLOTS), cases, targets


@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_decode_probes(G, KVH, monkeypatch):
    """Every segment's first and last key under splits 2, 4, 8 and 32,
    kv_len - 1, lo_tok and both ends of page-table entries 0, 32, 33, 255,
    256 and 511 come back bit for bit through every split and the merge; a
    key at kv_len or lo_tok - 1 leaves the uniform mean untouched."""
    run = _Run(monkeypatch)
    Hq = G * KVH
    h = ao.probe_codes()
    cpu, cases, targets = _probe_decode_pool(G, KVH)
    pool = cpu.to(DEV)
    kvh = torch.arange(Hq) // G
    n_pos = 0
    for W in (0,) + ao.LONG_WINDOWS:
        seqs, lens, qs, want = [], [], [], []
        for i, (n, w) in enumerate(cases):
            if w != W:
                continue
            tg, code = ao.long_probe_rows(targets[i], Hq)
            seqs += [i] * len(tg)
            lens += [n] * len(tg)
            qs.append(h[code])
            want.append(cpu.V[i][tg, kvh.expand_as(tg)])
        n_rows = len(seqs)
        for i, (n, w) in enumerate(cases):
            if w == W:
                seqs.append(len(cases) + i)
                lens.append(n)
                qs.append(h[0].expand(1, Hq, ao.D))
        q = torch.cat(qs).bfloat16()
        want = torch.cat(want)
        assert len(seqs) < SLOTS
        truth, _ = ao.oracle_batch(cpu, q[n_rows:], seqs[n_rows:],
                                   lens[n_rows:], window=W)
        decoy = torch.stack([cpu.V[s][n].repeat_interleave(G, dim=0)
                             for s, n in zip(seqs[n_rows:], lens[n_rows:])])
        meta = pool.meta(seqs, lens, window=W, max_kv=ao.LONG_WINDOW_CTX)
        for tag, got in run.sweep(q.to(DEV), pool, meta):
            bad = (got[:n_rows] != want).any(-1)
            assert not bad.any(), \
                (W, tag, int(bad.sum()), "of", bad.numel(),
                 bad.nonzero()[:4].tolist())
            neg = got[n_rows:]
            assert ao.ratio(neg, truth, per_vector=True) <= 1.0, (W, tag)
            assert not (neg == decoy).all(-1).any(), \
                (W, tag, "an invisible key was returned")
        n_pos += n_rows * Hq
    assert n_pos >= 200


@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_prefill_probes(G, KVH):
    """The same exact probe through k_prefill_attn: a fresh 16-tile chunk,
    chunks continued 3584, 4064 and 8191 keys in, and both windows on the
    4200-key sequence; negative probes sit at p + 1 of the last row and at
    p - W of the first."""
    Hq = G * KVH
    h = ao.probe_codes()
    pos, neg = ao.long_prefill_probe_cases()
    kvs, tgs, codes = [], [], []
    for i, (ql, n, W) in enumerate(pos):
        kv, tg, code = ao.long_prefill_probe_seq(ql, n, W, Hq, KVH, 700 + i)
        kvs.append(kv)
        tgs.append(tg)
        codes.append(code)
    n_negkeys = 0
    for i, (ql, n, W) in enumerate(neg):
        K, V = ao.long_probe_kv(n + 1, KVH, [], seed=720 + i)
        at = ao.long_prefill_neg_keys(ql, n, W)
        n_negkeys += len(at)
        K[torch.tensor(at)] = (32 * h[0]).bfloat16()
        kvs.append((K, V))
    assert n_negkeys == 4           # p - W exists at W = 1024 only
    cpu = ao.build_pool(kvs, seed=70 + G, max_ctx=ao.LONG_WINDOW_CTX)
    pool = cpu.to(DEV)
    kvh = torch.arange(Hq) // G
    for W in (0,) + ao.LONG_WINDOWS:
        pi = [i for i, c in enumerate(pos) if c[2] == W]
        ni = [i for i, c in enumerate(neg) if c[2] == W]
        seqs = pi + [len(pos) + i for i in ni]
        qls = [pos[i][0] for i in pi] + [neg[i][0] for i in ni]
        kls = [pos[i][1] for i in pi] + [neg[i][1] for i in ni]
        n_rows = sum(pos[i][0] for i in pi)
        q = torch.cat([h[codes[i]] for i in pi]
                      + [h[0].expand(neg[i][0], Hq, ao.D) for i in ni]) \
            .bfloat16()
        want = torch.cat([cpu.V[i][tgs[i], kvh.expand_as(tgs[i])]
                          for i in pi])
        truth, absp = ao.oracle_batch(cpu, q[n_rows:], seqs[len(pi):],
                                      kls[len(pi):], qls[len(pi):], W)
        got, _ = _prefill(q.to(DEV), pool, pool.meta(seqs, kls, qls, W))
        bad = (got[:n_rows] != want).any(-1)
        assert not bad.any(), (W, int(bad.sum()), "of", bad.numel(),
                               bad.nonzero()[:4].tolist())
        assert ao.ratio(got[n_rows:], truth, absp, per_vector=True) <= 1.0, W
    # one key on a row's edge, a batch of its own: the row it is the first
    # invisible key of keeps the uniform mean, its neighbour returns it
    wq, wn = ao.LONG_PREFILL_WINDOW_CASE
    for i, (W, key, blind, seeing) in enumerate(ao.LONG_PREFILL_EDGE):
        K, V = ao.long_probe_kv(wn, KVH, [key], seed=740 + i)
        cpu = ao.build_pool([(K, V)], seed=75 + i, max_ctx=ao.LONG_CTX)
        q = h[0].expand(wq, Hq, ao.D).bfloat16()
        truth, absp = ao.oracle_batch(cpu, q, [0], [wn], [wq], W)
        pool = cpu.to(DEV)
        got, _ = _prefill(q.to(DEV), pool, pool.meta([0], [wn], [wq], W))
        assert ao.ratio(got, truth, absp, per_vector=True) <= 1.0, (W, key)
        hit = V[key].repeat_interleave(G, dim=0)
        assert torch.equal(got[seeing], hit), (W, key, "neighbour row")
        assert not (got[blind] == hit).all(-1).any(), (W, key, "edge row")


# ---------------------------------------------------------------------------
# real-valued tier


def _fp8_twin(cpu):
    """An fp8 cache holding the codes of a (snapped) bf16 pool."""
    c = cpu.cache
    f = PagedKVCache(ao.LAYERS, c.n_kv_heads, ao.D, page_size=c.page_size,
                     n_pages=c.n_pages, max_slots=c.max_slots,
                     max_ctx=c.max_ctx, device=DEV, kv_quant="fp8")
    f.page_table.copy_(c.page_table)
    f.k_pool.copy_(quant.kv_fp8_encode(c.k_pool))
    f.v_pool.copy_(quant.kv_fp8_encode(c.v_pool))
    return ao.Pool(f, cpu.slots, cpu.K, cpu.V)


def _snap(kvs):
    return [tuple(quant.kv_fp8_decode(quant.kv_fp8_encode(t), torch.bfloat16)
                  for t in kv) for kv in kvs]


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_decode_real(G, KVH, fp8, monkeypatch):
    """N(0,1) inputs at 1025, 4096 and 8191 keys, full causal and both
    windows, against fused_oracle.assert_bf16_close unchanged.  fp8: the
    e4m3 pool is bit-equal to the bf16 instantiation on the decoded values
    and both are held to the oracle of those values."""
    run = _Run(monkeypatch)
    lens = ao.LONG_REAL_LENS
    S = len(lens)
    kvs = ao.real_kv(lens, KVH, ao.case_seed(G, KVH, 80))
    if fp8:
        kvs = _snap(kvs)
    cpu = ao.build_pool(kvs, seed=80, max_ctx=ao.LONG_CTX)
    pool = cpu.to(DEV)
    twin = _fp8_twin(cpu) if fp8 else None
    worst = 0.0
    for W in (0,) + ao.LONG_WINDOWS:
        for scale in ao.Q_SCALES:
            q = ao.real_q(S, G * KVH, scale, ao.case_seed(G, KVH, 81) + W)
            truth, _ = ao.oracle_batch(cpu, q, range(S), lens, window=W)
            qd = q.to(DEV)
            if scale != 1.0:
                qd = ao.strided(qd, KVH)
            meta = pool.meta(range(S), lens, window=W, max_kv=ao.LONG_CTX)
            for split, blk in ((None, "0"), (1, "0"), (_blk_split(G), "1")):
                got = run.decode(qd, pool, meta, split, blk)
                what = f"W{W} x{scale} split {split} blk {blk}"
                worst = max(worst, ao.assert_close(got, truth, [1] * S,
                                                   what=what))
                if fp8:
                    got8 = run.decode(qd, twin, meta, split, blk)
                    assert torch.equal(got8, got), what + ": fp8 != twin"
    _report(f"decode {'fp8' if fp8 else 'bf16'} G={G} KVH={KVH}", worst)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_prefill_real(G, KVH, fp8):
    """(1000, 1000) fresh, (512, 4096) continued and the 300-row chunk of
    the 4200-key sequence, full causal and both windows, against the
    decode budget plus 2^-9 softmax(S) @ |V|."""
    from ollamamq_amd.ops import hip
    hip.require()
    cases = ao.LONG_REAL_PREFILL + (ao.LONG_PREFILL_WINDOW_CASE,)
    qls, lens = [a for a, _ in cases], [b for _, b in cases]
    n = len(cases)
    kvs = ao.real_kv(lens, KVH, ao.case_seed(G, KVH, 90))
    if fp8:
        kvs = _snap(kvs)
    cpu = ao.build_pool(kvs, seed=90, max_ctx=ao.LONG_CTX)
    pool = cpu.to(DEV)
    twin = _fp8_twin(cpu) if fp8 else None
    worst = 0.0
    for W in (0,) + ao.LONG_WINDOWS:
        for scale in ao.Q_SCALES:
            q = ao.real_q(sum(qls), G * KVH, scale,
                          ao.case_seed(G, KVH, 91) + W)
            truth, absp = ao.oracle_batch(cpu, q, range(n), lens, qls, W)
            qd = q.to(DEV)
            if scale != 1.0:
                qd = ao.strided(qd, KVH)
            got, _ = _prefill(qd, pool, pool.meta(range(n), lens, qls, W))
            worst = max(worst, ao.assert_close(got, truth, qls, absp,
                                               what=f"W{W} x{scale}"))
            if fp8:
                got8, _ = _prefill(qd, twin, twin.meta(range(n), lens, qls,
                                                       W))
                assert torch.equal(got8, got), f"W{W} x{scale}: fp8 != twin"
    _report(f"prefill {'fp8' if fp8 else 'bf16'} G={G} KVH={KVH}", worst)


# ---------------------------------------------------------------------------
# mixed


@pytest.mark.parametrize("window", (0,) + ao.LONG_WINDOWS)
@pytest.mark.parametrize("G,KVH", [(4, 2), (7, 2)])
def test_mixed(G, KVH, window):
    """attention_mixed: decode rows of 2049 and 8191 keys, a fresh chunk of
    512 rows and one of 512 rows continued at 3584.  Real-valued inputs held
    to the oracle and bit-equal to the separate attention_decode /
    attention_prefill calls, then the same batch in the counting tier."""
    from ollamamq_amd.ops import hip
    hip.require()
    nd = len(ao.LONG_MIXED_DECODE)
    lens = list(ao.LONG_MIXED_DECODE) + [b for _, b in ao.LONG_MIXED_PREFILL]
    qls = [1] * nd + [a for a, _ in ao.LONG_MIXED_PREFILL]
    n = len(lens)
    seed = ao.case_seed(G, KVH, 95)
    cpu = ao.build_pool(ao.real_kv(lens, KVH, seed), seed=95,
                        max_ctx=ao.LONG_CTX)
    pool = cpu.to(DEV)
    q = ao.real_q(sum(qls), G * KVH, 1.0, seed + 1)
    truth, absp = ao.oracle_batch(cpu, q, range(n), lens, qls, window)
    qd = q.to(DEV)
    meta = pool.meta(range(n), lens, qls, window, mode="mixed", n_decode=nd)
    got = hip.attention_mixed(qd, pool.cache, ao.LAYER, meta).cpu()
    worst = ao.assert_close(got[:nd], truth[:nd], [1] * nd,
                            what="decode rows")
    worst = max(worst, ao.assert_close(got[nd:], truth[nd:], qls[nd:],
                                       absp[nd:], what="prefill rows"))
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
    # the same batch in the counting tier, both patterns
    for pattern in (0, 1):
        cpu = ao.build_pool(ao.counting_kv_long(lens, KVH, pattern),
                            seed=96 + pattern, max_ctx=ao.LONG_CTX)
        truth, _ = ao.oracle_batch(cpu, q, range(n), lens, qls, window)
        pool = cpu.to(DEV)
        meta = pool.meta(range(n), lens, qls, window, mode="mixed",
                         n_decode=nd)
        got = hip.attention_mixed(qd, pool.cache, ao.LAYER, meta).cpu()
        ao.assert_counting_long(got, truth, f"mixed counting {pattern}")


# ---------------------------------------------------------------------------
# one model-level case at length


@pytest.mark.parametrize("name", mo.LONG_CONFIGS)
def test_model_long(name):
    """RoPE, append and attention together past position 516: one sequence
    prefilled to 2100 tokens in chunks of 512 on a scrambled max_ctx = 4096
    cache, then three decode steps at B = 5 beside four short rows through
    the generic path and the fused chain, with the eager and the capture
    attention geometry.  Budgets are model_oracle's rule unchanged (2 x the
    CPU bf16 reference's worst rel / mx against the fp64 oracle at the same
    tokens); logits at chunk ends and decode rows, every live K/V row of
    every layer, nothing outside the owned rows touched."""
    from test_model_forward_gpu import gpu_model
    seqs, truth, budget = mo.truth_of(name, "long", mo.LONG_LENS)
    b = budget.fresh()
    rig = mo.Rig(gpu_model(name), seqs, DEV, seed=7,
                 max_ctx=mo.LONG_MAX_CTX)
    assert rig.kv.max_ctx == mo.LONG_MAX_CTX
    for a, e in mo.long_chunks():
        logits, rows = rig.forward([(0, a, e)], "prefill")
        assert rows == [(0, e - 1)]
        rig.check(truth, b, logits, rows, f"chunk {a}..{e}")
    ctx = (mo.LONG_PROMPT,) + mo.LONG_SHORT_CTX
    logits, rows = rig.forward(
        [(i, 0, c) for i, c in enumerate(ctx) if i], "prefill")
    rig.check(truth, b, logits, rows, "short rows")
    state = rig.save()
    for fused in (False, True):
        for capture in (False, True):
            rig.restore(state)
            for k in range(mo.LONG_STEPS):
                logits, rows = rig.forward(
                    [(i, c + k, c + k + 1) for i, c in enumerate(ctx)],
                    "decode", fused=fused, capture=capture)
                assert logits.shape[0] == len(ctx)
                rig.check(truth, b, logits, rows,
                          f"step {k} fused={fused} capture={capture}")
    lg, kv = b.report()
    lim = b.lim["logits"]
    print(f"BUDGET long {name}: logits rel {lim[0]:.4f} mx {lim[1]:.4f}")
    print(f"RATIO long {name} logits {lg:.3f} kv "
          + " ".join(f"{x:.3f}" for x in kv))
