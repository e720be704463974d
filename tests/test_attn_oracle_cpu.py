"""Soundness of the attention test helpers (tests/attn_oracle.py): the
adversarial pool, the fp64 oracle, the budgets and the exact tiers.  An fp32
emulation of each kernel's arithmetic must sit inside its tier's budget at
every shape the GPU tests use, the probe and counting inputs must come out
exact, and the assertions must notice a single missing or extra key, so a
GPU failure means the kernel, not the yardstick.  No GPU needed.
"""
import pytest
import torch

import attn_oracle as ao
import fused_oracle as fo
from ollamamq_amd.ops import reference as ref

GROUP_IDS = [f"G{G}-KVH{K}" for G, K in ao.GROUPS]


def _report(group, worst):
    print(f"[attn-oracle-cpu] {group}: worst normalised error {worst:.3f}")


# ---------------------------------------------------------------------------
# pool and oracle


def test_pool_is_adversarial():
    lens = (1, 17, 64, 200)
    kvs = ao.real_kv(lens, 2, seed=3)
    pool = ao.build_pool(kvs, seed=3)
    c = pool.cache
    n = len(lens)
    assert pool.slots != list(range(n)) and len(set(pool.slots)) == n
    assert 0 < ao.LAYER < ao.LAYERS - 1
    owned = torch.zeros(c.n_pages, ao.PAGE, dtype=torch.bool)
    for i, L in enumerate(lens):
        pages = c.page_table[pool.slots[i], :(L + 15) // 16].tolist()
        assert len(pages) < 2 or pages != sorted(pages)
        for p in range(L):
            assert not owned[pages[p // 16], p % 16]
            owned[pages[p // 16], p % 16] = True
            assert torch.equal(c.k_pool[ao.LAYER, pages[p // 16], :, p % 16],
                               kvs[i][0][p])
            assert torch.equal(c.v_pool[ao.LAYER, pages[p // 16], :, p % 16],
                               kvs[i][1][p])
    for pool_t in (c.k_pool, c.v_pool):
        nan = torch.isnan(pool_t).all(dim=-1).all(dim=2)   # [L, page, off]
        for layer in range(ao.LAYERS):
            want = ~owned if layer == ao.LAYER else torch.ones_like(owned)
            assert torch.equal(nan[layer], want)
        fin = torch.isfinite(pool_t).all(dim=-1).all(dim=2)
        assert torch.equal(fin[ao.LAYER], owned)
    # every page-table entry that is not an owned page is the NaN spare
    mask = torch.ones_like(c.page_table, dtype=torch.bool)
    for i, L in enumerate(lens):
        mask[pool.slots[i], :(L + 15) // 16] = False
    spare = c.page_table[mask].unique()
    assert spare.numel() == 1
    assert torch.isnan(c.k_pool[:, int(spare)]).all()


@pytest.mark.parametrize("window", [0, 1, 70])
def test_oracle_matches_fp32_reference(window):
    G, KVH = 3, 2
    # decode rows
    kvs = ao.real_kv(ao.DECODE_LENS, KVH, seed=11)
    pool = ao.build_pool(kvs, seed=11)
    S = len(ao.DECODE_LENS)
    q = ao.real_q(S, G * KVH, 1.0, seed=11)
    meta = pool.meta(range(S), ao.DECODE_LENS, window=window)
    got = ref.attention(q.float(), pool.cache, ao.LAYER, meta)
    want, _ = ao.oracle_batch(pool, q, range(S), ao.DECODE_LENS,
                              window=window)
    assert float((got.double() - want).abs().max()) <= 1e-5
    # prefill chunks, continued ones included
    qls = [a for a, _ in ao.PREFILL_CASES]
    kls = [b for _, b in ao.PREFILL_CASES]
    pool = ao.build_pool(ao.real_kv(kls, KVH, seed=12), seed=12)
    q = ao.real_q(sum(qls), G * KVH, 1.0, seed=12)
    meta = pool.meta(range(len(kls)), kls, qls, window=window)
    got = ref.attention(q.float(), pool.cache, ao.LAYER, meta)
    want, absp = ao.oracle_batch(pool, q, range(len(kls)), kls, qls,
                                 window=window)
    assert float((got.double() - want).abs().max()) <= 1e-5
    assert bool((absp >= want.abs() - 1e-12).all())


def test_ratio_is_the_fused_oracle_budget():
    t = torch.randn(5, 4, 128, generator=torch.Generator().manual_seed(0),
                    dtype=torch.float64)
    g = (t * (1 + 2.0 ** -9)).float()
    assert abs(ao.ratio(g, t) - fo.assert_bf16_close(g, t)) < 1e-12
    assert ao.ratio(torch.full_like(g, float("nan")), t) == float("inf")
    # the prefill term only ever adds to the budget
    assert ao.ratio(g, t, absP=t.abs()) < ao.ratio(g, t)


def test_probe_gap_condition():
    h = ao.probe_codes()
    assert h.shape == (ao.N_CODES, ao.D) and bool((h.abs() == 1).all())
    gram = h @ h.t()
    assert bool((gram.diagonal() == ao.D).all())
    gram.fill_diagonal_(0)
    gap = (32 * ao.D - 32 * float(gram.abs().max())) * ao.SCALE
    assert gap >= ao.MIN_GAP
    # exp(-gap) is 0 in fp32: every non-target probability vanishes
    assert float(torch.exp(torch.tensor(-ao.MIN_GAP))) == 0.0
    # within one (sequence, kv head) no code repeats
    pos = torch.arange(ao.PROBE_CAP)
    for s in range(ao.PROBE_SEQS):
        for k in range(3):
            assert ao._code_of(s, k, pos).unique().numel() == ao.PROBE_CAP


# ---------------------------------------------------------------------------
# tier B: an fp32 emulation of each kernel stays inside its budget


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_emulated_decode_within_budget(G, KVH):
    Hq = G * KVH
    worst = 0.0
    for gi, (tag, lens, W, splits, max_kv) in enumerate(ao.decode_groups(G)):
        splits = [ao.wrapper_split(len(lens), KVH, max_kv, s) for s in splits]
        assert tag != "capture" or splits == [32]
        for scale in ao.Q_SCALES:
            kvs, q = ao.decode_inputs(G, KVH, gi, lens, scale)
            for i, n in enumerate(lens):
                K, V = kvs[i]
                truth, _ = ao.attention_oracle(q[i:i + 1], K, V, [n - 1], n,
                                               W)
                for CH in ao.DECODE_CHUNKS:
                    for split in splits:
                        got = ao.emulate_decode(q[i], K, V, n, W, CH, split)
                        w = ao.ratio(got.unsqueeze(0), truth)
                        assert w <= 1.0, (tag, scale, n, CH, split, w)
                        worst = max(worst, w)
                        if W == 1:
                            rep = V[n - 1].repeat_interleave(G, dim=0)
                            assert torch.equal(got, rep)
    _report(f"decode G={G} KVH={KVH}", worst)
    # the budget is not slack by an order of magnitude either
    assert worst >= 0.05


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_emulated_prefill_within_budget(G, KVH):
    Hq = G * KVH
    worst_mfma = worst_valu = 0.0
    for wi, (W, cases) in enumerate(ao.prefill_runs()):
        for scale in ao.Q_SCALES:
            kvs, q_all = ao.prefill_inputs(G, KVH, wi, cases, scale)
            at = 0
            for i, (ql, n) in enumerate(cases):
                q = q_all[at:at + ql]
                at += ql
                K, V = kvs[i]
                truth, absp = ao.attention_oracle(
                    q, K, V, list(range(n - ql, n)), n, W)
                for CH in (32, 64):
                    got = ao.emulate_prefill(q, K, V, n - ql, W, CH)
                    w = ao.ratio(got, truth, absp)
                    assert w <= 1.0, ("mfma", W, scale, ql, n, CH, w)
                    worst_mfma = max(worst_mfma, w)
                if W == 0:       # the VALU kernel keeps p in fp32
                    got = ao.emulate_prefill(q, K, V, n - ql, 0, 64,
                                             round_p=False)
                    w = ao.ratio(got, truth)
                    assert w <= 1.0, ("valu", scale, ql, n, w)
                    worst_valu = max(worst_valu, w)
                if W == 1:
                    rep = V[n - ql:n].repeat_interleave(G, dim=1)
                    assert torch.equal(ao.emulate_prefill(q, K, V, n - ql,
                                                          1), rep)
    _report(f"prefill G={G} KVH={KVH}", worst_mfma)
    _report(f"valu prefill G={G} KVH={KVH}", worst_valu)


# ---------------------------------------------------------------------------
# tier A1: probes are exact under the emulation and notice their key


def _one_hot_vis(vis, Hq, targets, add):
    """vis [Q, n] -> [Hq, Q, n] with each (row, head)'s target key removed
    (add False) or admitted (add True)."""
    v = vis.unsqueeze(0).repeat(Hq, 1, 1)
    tg = torch.tensor(targets).t()                     # [Hq, Q]
    v.scatter_(2, tg.unsqueeze(-1), add)
    return v


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_decode_probes(G, KVH):
    Hq = G * KVH
    kvs = ao.probe_kv(KVH)
    pool = ao.build_pool(kvs, seed=1, max_ctx=512)
    n_pos = n_neg = 0
    for W in ao.PROBE_DECODE_WINDOWS:
        seqs, lens, targets, positive = ao.decode_probe_plan(Hq, KVH, W)
        S = len(seqs)
        q = ao.probe_queries(seqs, [1] * S, targets, Hq, KVH)
        want = ao.probe_expected(pool, seqs, [1] * S, targets, Hq)
        pos = torch.tensor(positive)
        for r in range(S):
            K, V = kvs[seqs[r]]
            n = lens[r]
            lo = n - W if (W > 0 and n > W) else 0
            for h in range(Hq):
                t = targets[r][h]
                assert (lo <= t < n) == positive[r][h]
            truth, _ = ao.attention_oracle(q[r:r + 1], K, V, [n - 1], n, W)
            # the oracle itself is one-hot on positive probes
            assert torch.equal(truth[0][pos[r]].bfloat16(), want[r][pos[r]])
            for CH in ao.DECODE_CHUNKS:
                for split in (1, 3, 5):
                    got = ao.emulate_decode(q[r], K, V, n, W, CH, split)
                    assert torch.equal(got[pos[r]], want[r][pos[r]]), \
                        (W, n, CH, split, targets[r])
                    neg = ~pos[r]
                    if neg.any():
                        assert ao.ratio(got[neg], truth[0][neg],
                                        per_vector=True) <= 1.0
                        assert not (got[neg] == want[r][neg]).all(-1).any()
            # sensitivity: without its target a positive probe no longer
            # returns V[t]; with the invisible key admitted a negative
            # probe leaves the budget
            vis = ao.visible([n - 1], n, W, K.shape[0])
            cut, _ = ao.attention_oracle(
                q[r:r + 1], K, V, None, n, W,
                vis=_one_hot_vis(vis, Hq, [targets[r]], False))
            add, _ = ao.attention_oracle(
                q[r:r + 1], K, V, None, n, W,
                vis=_one_hot_vis(vis, Hq, [targets[r]], True))
            for h in range(Hq):
                if positive[r][h]:
                    n_pos += 1
                    if n > 1 and (W != 1):
                        assert not torch.equal(cut[0, h].bfloat16(),
                                               want[r, h])
                else:
                    n_neg += 1
                    assert ao.ratio(add[0, h], truth[0, h],
                                    per_vector=True) > 1.0
    assert n_pos >= 100 and n_neg >= 20


@pytest.mark.parametrize("G,KVH", ao.GROUPS, ids=GROUP_IDS)
def test_prefill_probes(G, KVH):
    Hq = G * KVH
    kvs = ao.probe_kv(KVH)
    pool = ao.build_pool(kvs, seed=1, max_ctx=512)
    n_neg = 0
    for W, cases in [(0, ao.PREFILL_CASES)] + \
            [(W, ao.PREFILL_WINDOW_CASES) for W in ao.PROBE_PREFILL_WINDOWS[1:]]:
        seqs, lens, qls, targets, positive = ao.prefill_probe_plan(
            Hq, cases, W)
        q = ao.probe_queries(seqs, qls, targets, Hq, KVH)
        want = ao.probe_expected(pool, seqs, qls, targets, Hq)
        pos = torch.tensor(positive)
        truth, absp = ao.oracle_batch(pool, q, seqs, lens, qls, W)
        assert torch.equal(truth[pos].bfloat16(), want[pos])
        at = 0
        for s, n, ql in zip(seqs, lens, qls):
            K, V = kvs[s]
            sl = slice(at, at + ql)
            got = ao.emulate_prefill(q[sl], K, V, n - ql, W)
            p, ng = pos[sl], ~pos[sl]
            assert torch.equal(got[p], want[sl][p]), (W, ql, n)
            if ng.any():
                assert ao.ratio(got[ng], truth[sl][ng], absp[sl][ng],
                                per_vector=True) <= 1.0
                assert not (got[ng] == want[sl][ng]).all(-1).any()
            # sensitivity, as for decode
            vis = ao.visible(list(range(n - ql, n)), n, W, K.shape[0])
            add, _ = ao.attention_oracle(
                q[sl], K, V, None, n, W,
                vis=_one_hot_vis(vis, Hq, targets[sl], True))
            cut, _ = ao.attention_oracle(
                q[sl], K, V, None, n, W,
                vis=_one_hot_vis(vis, Hq, targets[sl], False))
            for r in range(ql):
                for h in range(Hq):
                    if positive[at + r][h]:
                        # a lone visible key has nothing to fall back on
                        if int(vis[r].sum()) > 1:
                            assert not torch.equal(
                                cut[r, h].bfloat16(), want[at + r, h])
                    else:
                        n_neg += 1
                        assert ao.ratio(
                            add[r, h], truth[at + r, h], absp[at + r, h],
                            per_vector=True) > 1.0
            at += ql
    assert n_neg >= 50


# ---------------------------------------------------------------------------
# tier A2: counting inputs are inside budget under the emulation, and one
# key more or less is not


def _count_truth(V, kvh_rep, vis_row):
    """c_d / n for one query row: V [n, KVH, 128], vis_row [n] bool."""
    c = V[vis_row].double().sum(dim=0)                 # [KVH, 128]
    return (c / int(vis_row.sum())).repeat_interleave(kvh_rep, dim=0)


@pytest.mark.parametrize("KVH", [1, 2, 3])
def test_decode_counting(KVH):
    G = 2
    Hq = G * KVH
    kvs = ao.counting_kv(KVH)
    runs = [(0, ao.COUNT_DECODE_LENS)] + list(ao.DECODE_WINDOWS)
    for W, lens in runs:
        q = ao.real_q(len(lens), Hq, 1.0, seed=W + 5)
        for r, n in enumerate(lens):
            K, V = kvs[r % ao.COUNT_SEQS]
            vis = ao.visible([n - 1], n, W, K.shape[0])
            truth, _ = ao.attention_oracle(q[r:r + 1], K, V, [n - 1], n, W)
            assert torch.allclose(truth[0], _count_truth(V, G, vis[0]),
                                  rtol=0, atol=1e-15)
            for CH in ao.DECODE_CHUNKS:
                for split in (1, 2, 3, 5, 32):
                    got = ao.emulate_decode(q[r], K, V, n, W, CH, split)
                    ao.assert_counting(got.unsqueeze(0), truth,
                                       f"W{W} n{n} CH{CH} split{split}")
            # every single deletion, and the two possible admissions
            keys = vis[0].nonzero().flatten().tolist()
            lo = keys[0]
            edits = [(k, False) for k in keys if len(keys) > 1]
            edits += [(k, True) for k in (n, lo - 1) if k >= 0]
            ev = vis.repeat(len(edits), 1)
            for e, (k, add) in enumerate(edits):
                ev[e, k] = add
            wrong, _ = ao.attention_oracle(
                q[r:r + 1].expand(len(edits), -1, -1), K, V, None, n, W,
                vis=ev)
            for e in range(len(edits)):
                with pytest.raises(AssertionError):
                    ao.assert_counting(wrong[e:e + 1], truth)


@pytest.mark.parametrize("KVH", [1, 2, 3])
def test_prefill_counting(KVH):
    G = 2
    Hq = G * KVH
    kvs = ao.counting_kv(KVH)
    runs = [(0, ao.PREFILL_CASES)] + \
        [(W, ao.PREFILL_WINDOW_CASES) for W in ao.PREFILL_WINDOWS]
    for W, cases in runs:
        for i, (ql, n) in enumerate(cases):
            K, V = kvs[i % ao.COUNT_SEQS]
            q = ao.real_q(ql, Hq, 1.0, seed=W + i)
            qpos = list(range(n - ql, n))
            vis = ao.visible(qpos, n, W, K.shape[0])
            truth, _ = ao.attention_oracle(q, K, V, qpos, n, W)
            got = ao.emulate_prefill(q, K, V, n - ql, W)
            ao.assert_counting(got, truth, f"W{W} {ql},{n}")
            # per row: drop the first, a middle and the last visible key,
            # admit p + 1 (or kv_len) and p - W
            for r in range(0, ql, max(1, ql // 7)):
                keys = vis[r].nonzero().flatten().tolist()
                edits = [(k, False) for k in
                         {keys[0], keys[len(keys) // 2], keys[-1]}
                         if len(keys) > 1]
                edits += [(k, True) for k in (qpos[r] + 1, keys[0] - 1)
                          if k >= 0]
                ev = vis[r:r + 1].repeat(len(edits), 1)
                for e, (k, add) in enumerate(edits):
                    ev[e, k] = add
                wrong, _ = ao.attention_oracle(
                    q[r:r + 1].expand(len(edits), -1, -1), K, V, None, n, W,
                    vis=ev)
                for e in range(len(edits)):
                    with pytest.raises(AssertionError):
                        ao.assert_counting(wrong[e:e + 1], truth[r:r + 1])
