"""Soundness of the long-context attention yardsticks of
tests/attn_oracle.py, at the shapes tests/test_attention_long_gpu.py runs:
the counting assertion passes for an fp32 emulation of the kernels and
fails for every single missing key and every first invisible key admitted,
the single-target probes come out bit-exact under the emulation, and the
emulation of the real-valued tier stays inside the project's two budgets,
which are asserted unchanged.  No GPU needed.
"""
import pytest
import torch

import attn_oracle as ao

GROUP_IDS = [f"G{G}-KVH{K}" for G, K in ao.LONG_GROUPS]


def _report(group, worst):
    print(f"[attn-long-cpu] {group}: worst fraction of budget {worst:.3f}")


def test_long_pool_is_adversarial():
    lens = (513, 4096, 8192)
    kvs = ao.real_kv(lens, 2, seed=5)
    pool = ao.build_pool(kvs, seed=5, max_ctx=ao.LONG_CTX)
    c = pool.cache
    owned = torch.zeros(c.n_pages, ao.PAGE, dtype=torch.bool)
    free = torch.ones_like(c.page_table, dtype=torch.bool)
    for i, n in enumerate(lens):
        need = (n + ao.PAGE - 1) // ao.PAGE
        pt = c.page_table[pool.slots[i], :need]
        assert pt.tolist() != sorted(pt.tolist())
        free[pool.slots[i], :need] = False
        pos = torch.arange(n)
        pg, off = pt[pos // ao.PAGE].long(), pos % ao.PAGE
        assert not owned[pg, off].any()
        owned[pg, off] = True
        assert torch.equal(c.k_pool[ao.LAYER, pg, :, off], kvs[i][0])
        assert torch.equal(c.v_pool[ao.LAYER, pg, :, off], kvs[i][1])
    assert int(owned.sum()) == sum(lens)
    for t in (c.k_pool, c.v_pool):
        nan = torch.isnan(t).all(dim=-1).all(dim=2)        # [L, page, off]
        for layer in range(ao.LAYERS):
            want = ~owned if layer == ao.LAYER else torch.ones_like(owned)
            assert torch.equal(nan[layer], want)
    spare = c.page_table[free].unique()
    assert spare.numel() == 1 and torch.isnan(c.k_pool[:, int(spare)]).all()
    assert pool.slots != sorted(pool.slots) or pool.slots[0] != 0


# ---------------------------------------------------------------------------
# counting tier


def _count(V, vis_row):
    """c_d / n of one row: V [n, KVH, 128], vis_row [n] bool -> [KVH, 128]."""
    return V[vis_row].double().sum(dim=0) / int(vis_row.sum())


COUNT_RUNS = [(0, ao.LONG_DECODE_LENS)] + \
    [(W, ao.long_window_lens(W)) for W in ao.LONG_WINDOWS]


@pytest.mark.parametrize("pattern", [0, 1], ids=["mod128", "div128"])
@pytest.mark.parametrize("W,lens", COUNT_RUNS,
                         ids=[f"W{w}" for w, _ in COUNT_RUNS])
def test_decode_counting_long(W, lens, pattern):
    """At every length: the oracle is the count ratio, the emulation passes
    the assertion, every single deletion and both admissions fail it."""
    G, KVH = 2, 2
    kvs = ao.counting_kv_long(lens, KVH, pattern, extra=1)
    q = ao.real_q(len(lens), G * KVH, 1.0, seed=W + 5)
    for r, n in enumerate(lens):
        K, V = kvs[r]
        vis = ao.visible([n - 1], n, W, n + 1)[0]
        truth, _ = ao.attention_oracle(q[r:r + 1], K, V, [n - 1], n, W)
        t = _count(V, vis)                                 # [KVH, 128]
        assert torch.allclose(truth[0], t.repeat_interleave(G, dim=0),
                              rtol=0, atol=1e-12)
        for CH, split in ((32, 1), (32, 4), (64, 2), (64, 8), (64, 32)):
            got = ao.emulate_decode(q[r], K, V, n, W, CH, split)
            ao.assert_counting_long(got.unsqueeze(0), truth,
                                    f"n{n} CH{CH} split{split}")
        # every single deletion, as a kernel would emit it (bf16)
        keys = vis.nonzero().flatten()
        nv = keys.numel()
        c = V[vis].double().sum(dim=0)
        cut = ((c.unsqueeze(0) - V[keys].double()) / (nv - 1)).bfloat16()
        ok = ao.counting_long_ok(cut, t.expand_as(cut))    # [nv, KVH]
        assert not ok.any(), (n, "deletions that pass", int(ok.sum()))
        # the two admissions
        lo = int(keys[0])
        for k in [n] + ([lo - 1] if lo > 0 else []):
            add = ((c + V[k].double()) / (nv + 1)).bfloat16()
            assert not ao.counting_long_ok(add, t).any(), (n, "admits", k)
        # the formula above is what the oracle gives for an edited mask
        for k, on in ((lo, False), (int(keys[nv // 2]), False),
                      (n - 1, False), (n, True)):
            ev = vis.clone().unsqueeze(0)
            ev[0, k] = on
            wrong, _ = ao.attention_oracle(q[r:r + 1], K, V, None, n, W,
                                           vis=ev)
            assert torch.allclose(wrong[0, ::G], _count(V, ev[0]), rtol=0,
                                  atol=1e-12)
            with pytest.raises(AssertionError):
                ao.assert_counting_long(wrong.bfloat16(), truth)


@pytest.mark.parametrize("pattern", [0, 1], ids=["mod128", "div128"])
def test_prefill_counting_long(pattern):
    G, KVH = 2, 1
    cases = [(a, b, 0) for a, b in
             ao.LONG_PREFILL_FRESH + ao.LONG_PREFILL_CONT] + \
        [ao.LONG_PREFILL_WINDOW_CASE + (W,) for W in ao.LONG_WINDOWS]
    kvs = ao.counting_kv_long([b for _, b, _ in cases], KVH, pattern,
                              extra=1)
    for i, (ql, n, W) in enumerate(cases):
        K, V = kvs[i]
        q = ao.real_q(ql, G * KVH, 1.0, seed=W + i)
        qpos = list(range(n - ql, n))
        vis = ao.visible(qpos, n, W, n + 1)
        truth, _ = ao.attention_oracle(q, K, V, qpos, n, W)
        got = ao.emulate_prefill(q, K, V, n - ql, W)
        ao.assert_counting_long(got, truth, f"W{W} {ql},{n}")
        # first, middle and last row and the rows around a tile edge:
        # every deletion, both admissions
        for r in sorted({0, 31, 32, 33, ql // 2, ql - 1} & set(range(ql))):
            keys = vis[r].nonzero().flatten()
            nv = keys.numel()
            c = V[vis[r]].double().sum(dim=0)
            t = truth[r, ::G]
            assert torch.allclose(t, c / nv, rtol=0, atol=1e-12)
            # div128 alone is blind while every key involved shares one
            # 128-block (the ratio is 1 whatever the count); mod128 is not
            lo = int(keys[0])
            one_block = pattern == 1 and lo // ao.D == (qpos[r] + 1) // ao.D
            assert not one_block or nv <= ao.D
            if nv > 1 and not one_block:
                cut = ((c.unsqueeze(0) - V[keys].double()) / (nv - 1)) \
                    .bfloat16()
                assert not ao.counting_long_ok(cut, t.expand_as(cut)).any()
            for k in [qpos[r] + 1] + ([lo - 1] if lo > 0 else []):
                if one_block and k // ao.D == lo // ao.D:
                    continue
                add = ((c + V[k].double()) / (nv + 1)).bfloat16()
                assert not ao.counting_long_ok(add, t).any(), (ql, n, r, k)


# ---------------------------------------------------------------------------
# single-target probes


def test_probe_scores_vanish():
    """The target scores 4096 / sqrt(128); a zero key sits 362 below it and
    another target key at least MIN_GAP below, and exp of either is 0."""
    top = 32 * ao.D * ao.SCALE
    assert abs(top - 362.04) < 0.01 and top >= ao.MIN_GAP
    ao.probe_codes()                      # asserts the pairwise gap
    assert float(torch.exp(torch.tensor(-ao.MIN_GAP))) == 0.0


@pytest.mark.parametrize("G,KVH", [(1, 2), (4, 2)], ids=["G1", "G4"])
def test_decode_probes_long(G, KVH):
    Hq = G * KVH
    CH = 32 if G == 1 else 64
    h = ao.probe_codes()
    kvh = torch.arange(Hq) // G
    n_pos = 0
    for i, (n, W) in enumerate(ao.long_decode_probe_cases()):
        if G == 1 and n > 2100:           # the sweep is per row in Python
            continue
        targets = ao.long_probe_targets(n, W, CH, (2, 4, 8, 32))
        lo = n - W if (W > 0 and n > W) else 0
        assert {lo, n - 1} <= set(targets) and \
            all(lo <= t < n for t in targets)
        for e in ao.LONG_PT_ENTRIES:
            for t in (e * ao.PAGE, e * ao.PAGE + ao.PAGE - 1):
                assert (t in targets) == (lo <= t < n)
        K, V = ao.long_probe_kv(n, KVH, targets, seed=600 + i)
        tg, code = ao.long_probe_rows(targets, Hq)
        q = h[code].bfloat16()
        want = V[tg, kvh.expand_as(tg)]
        rows = range(len(tg)) if n < 8000 else range(0, len(tg), 3)
        for r in rows:
            truth, _ = ao.attention_oracle(q[r:r + 1], K, V, [n - 1], n, W)
            assert torch.equal(truth[0].bfloat16(), want[r])
            for split in (4, 32):
                got = ao.emulate_decode(q[r], K, V, n, W, CH, split)
                assert torch.equal(got, want[r]), (n, W, split, r)
            n_pos += Hq
        # a probe whose target is cut from the mask returns something else
        vis = ao.visible([n - 1], n, W, n).repeat(Hq, 1, 1)
        vis[torch.arange(Hq), 0, tg[0]] = False
        cut, _ = ao.attention_oracle(q[:1], K, V, None, n, W, vis=vis)
        assert not (cut[0].bfloat16() == want[0]).all(-1).any()
        # negative: the only nonzero keys are invisible
        Kn, Vn = ao.long_probe_kv(n + 1, KVH, [], seed=620 + i)
        neg = [t for t in (n, lo - 1) if t >= 0]
        Kn[torch.tensor(neg)] = (32 * h[0]).bfloat16()
        qn = h[0].expand(1, Hq, ao.D).bfloat16()
        truth, _ = ao.attention_oracle(qn, Kn, Vn, [n - 1], n, W)
        mean = Vn[lo:n].double().mean(dim=0).repeat_interleave(G, dim=0)
        assert torch.allclose(truth[0], mean, rtol=0, atol=1e-12)
        got = ao.emulate_decode(qn[0], Kn, Vn, n, W, CH, 4)
        assert ao.ratio(got.unsqueeze(0), truth, per_vector=True) <= 1.0
        for k in neg:                     # admitted, it takes the output
            vis = ao.visible([n - 1], n, W, n + 1)
            vis[0, k] = True
            add, _ = ao.attention_oracle(qn, Kn, Vn, None, n, W, vis=vis)
            assert ao.ratio(add, truth, per_vector=True) > 1.0
    assert n_pos >= 100


def test_prefill_probes_long():
    G, KVH = 4, 2
    Hq = G * KVH
    h = ao.probe_codes()
    kvh = torch.arange(Hq) // G
    pos, neg = ao.long_prefill_probe_cases()
    for i, (ql, n, W) in enumerate(pos):
        (K, V), tg, code = ao.long_prefill_probe_seq(ql, n, W, Hq, KVH,
                                                     700 + i)
        qpos = torch.arange(n - ql, n).unsqueeze(1)
        lo = (qpos - W + 1).clamp_min(0) if W else torch.zeros_like(qpos)
        assert bool(((tg >= lo) & (tg <= qpos)).all())
        assert bool((tg == qpos).any()) and bool((tg == lo).any())
        q = h[code].bfloat16()
        want = V[tg, kvh.expand_as(tg)]
        truth, _ = ao.attention_oracle(q, K, V, qpos.flatten().tolist(), n,
                                       W)
        assert torch.equal(truth.bfloat16(), want)
        got = ao.emulate_prefill(q, K, V, n - ql, W)
        assert torch.equal(got, want), (ql, n, W)
    for i, (ql, n, W) in enumerate(neg):
        K, V = ao.long_probe_kv(n + 1, KVH, [], seed=720 + i)
        at = ao.long_prefill_neg_keys(ql, n, W)
        K[torch.tensor(at)] = (32 * h[0]).bfloat16()
        q = h[0].expand(ql, Hq, ao.D).bfloat16()
        qpos = list(range(n - ql, n))
        vis = ao.visible(qpos, n, W, n + 1)
        assert not vis[:, at].any()
        truth, absp = ao.attention_oracle(q, K, V, qpos, n, W)
        got = ao.emulate_prefill(q, K, V, n - ql, W)
        assert ao.ratio(got, truth, absp, per_vector=True) <= 1.0
        for k in at:
            ev = vis.clone()
            ev[:, k] = True
            add, _ = ao.attention_oracle(q, K, V, None, n, W, vis=ev)
            assert ao.ratio(add, truth, absp, per_vector=True) > 1.0


# ---------------------------------------------------------------------------
# real-valued tier: the fp32 emulation inside the unchanged budgets


@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_emulated_decode_long_within_budget(G, KVH):
    lens = ao.LONG_REAL_LENS
    CH = 32 if G == 1 else 64
    kvs = ao.real_kv(lens, KVH, ao.case_seed(G, KVH, 80))
    worst = 0.0
    for W in (0,) + ao.LONG_WINDOWS:
        for scale in ao.Q_SCALES:
            q = ao.real_q(len(lens), G * KVH, scale,
                          ao.case_seed(G, KVH, 81) + W)
            for i, n in enumerate(lens):
                K, V = kvs[i]
                truth, _ = ao.attention_oracle(q[i:i + 1], K, V, [n - 1], n,
                                               W)
                for split in (1, 2 if G == 8 else 4, 32):
                    got = ao.emulate_decode(q[i], K, V, n, W, CH, split)
                    w = ao.ratio(got.unsqueeze(0), truth)
                    assert w <= 1.0, (W, scale, n, split, w)
                    worst = max(worst, w)
    _report(f"decode G={G} KVH={KVH}", worst)


@pytest.mark.parametrize("G,KVH", ao.LONG_GROUPS, ids=GROUP_IDS)
def test_emulated_prefill_long_within_budget(G, KVH):
    cases = ao.LONG_REAL_PREFILL + (ao.LONG_PREFILL_WINDOW_CASE,)
    kvs = ao.real_kv([b for _, b in cases], KVH, ao.case_seed(G, KVH, 90))
    worst = 0.0
    for W in (0,) + ao.LONG_WINDOWS:
        for scale in ao.Q_SCALES:
            q_all = ao.real_q(sum(a for a, _ in cases), G * KVH, scale,
                              ao.case_seed(G, KVH, 91) + W)
            at = 0
            for i, (ql, n) in enumerate(cases):
                q = q_all[at:at + ql]
                at += ql
                K, V = kvs[i]
                truth, absp = ao.attention_oracle(
                    q, K, V, list(range(n - ql, n)), n, W)
                got = ao.emulate_prefill(q, K, V, n - ql, W)
                w = ao.ratio(got, truth, absp)
                assert w <= 1.0, (W, scale, ql, n, w)
                worst = max(worst, w)
    _report(f"prefill G={G} KVH={KVH}", worst)


def test_prefill_edge_probes_long():
    """One nonzero key on a row's edge: invisible to that row (uniform
    mean), returned bit for bit by the row beside it."""
    G, KVH = 4, 2
    Hq = G * KVH
    h = ao.probe_codes()
    ql, n = ao.LONG_PREFILL_WINDOW_CASE
    qpos = list(range(n - ql, n))
    for i, (W, key, blind, seeing) in enumerate(ao.LONG_PREFILL_EDGE):
        vis = ao.visible(qpos, n, W, n)
        assert not vis[blind, key] and vis[seeing, key]
        assert key in (qpos[blind] + 1, qpos[blind] - W)
        K, V = ao.long_probe_kv(n, KVH, [key], seed=740 + i)
        q = h[0].expand(ql, Hq, ao.D).bfloat16()
        truth, absp = ao.attention_oracle(q, K, V, qpos, n, W)
        got = ao.emulate_prefill(q, K, V, n - ql, W)
        assert ao.ratio(got, truth, absp, per_vector=True) <= 1.0
        hit = V[key].repeat_interleave(G, dim=0)
        assert torch.equal(got[seeing], hit)
        lo = max(0, qpos[blind] - W + 1) if W else 0
        mean = V[lo:qpos[blind] + 1].double().mean(0).repeat_interleave(
            G, dim=0)
        assert torch.allclose(truth[blind], mean, rtol=0, atol=1e-12)
        ev = vis.clone()
        ev[blind, key] = True
        add, _ = ao.attention_oracle(q, K, V, None, n, W, vis=ev)
        assert ao.ratio(add[blind], truth[blind], absp[blind],
                        per_vector=True) > 1.0
