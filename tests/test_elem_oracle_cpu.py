"""Soundness of the elementwise / sampler test helpers
(tests/elem_oracle.py): the counter-noise emulation and its inverse, the
uniform mapping over every mantissa the kernel can produce, the adversarial
append pool, the budgets (an fp32 round-once emulation of each formula must
sit inside them at every shape the GPU files use) and the Gumbel decision
margin.  No GPU needed.
"""
import numpy as np
import pytest
import torch

import attn_oracle as ao
import elem_oracle as eo
import fused_oracle as fo


# ---------------------------------------------------------------------------
# the counter noise


def _fmix_int(k):
    """murmur3 fmix64 in Python ints."""
    k ^= k >> 33
    k = k * 0xFF51AFD7ED558CCD & eo.M64
    k ^= k >> 33
    k = k * 0xC4CEB9FE1A85EC53 & eo.M64
    return k ^ (k >> 33)


def _u01_int(seed, ctr, v, nbits):
    """The whole chain in Python ints and exact fractions of 2^-(nbits+1)."""
    key = ((seed & eo.M64) * eo.GOLD & eo.M64) \
        ^ ((ctr & 0xFFFFFFFF) * eo.CTRMUL & eo.M64) ^ v
    m = _fmix_int(key) >> (64 - nbits)
    return m, (2 * m + 1) / 2.0 ** (nbits + 1)


def test_fmix64_matches_python_ints():
    keys = [0, 1, 0x0123456789ABCDEF, eo.M64, 1 << 63]
    got = eo.fmix64(np.array(keys, dtype=np.uint64))
    assert [int(g) for g in got] == [_fmix_int(k) for k in keys]
    assert int(got[0]) == 0                       # fmix64 fixes 0
    # a bijection: distinct keys, distinct hashes
    assert len({int(g) for g in got}) == len(keys)


@pytest.mark.parametrize("seed,ctr,v", [
    (0, 0, 0), (1, 1, 1), (-1, 2 ** 31 - 1, 128255),
    (2 ** 63 - 1, 4095, 50256), (-2 ** 63, 17, 5),
    (eo.POISON_SEED, 0, 5)])
def test_hash_u01_matches_python_ints(seed, ctr, v):
    m, u = _u01_int(seed, ctr, v, eo.U_BITS)
    got = eo.hash_u01(seed, ctr, v)
    assert got.dtype == np.float32 and got.shape == (1,)
    # (2m + 1) * 2^-24 is exact in float32 for m < 2^23
    assert float(got[0]) == u
    assert int(eo.hash_key(seed, ctr, v)[0]) >> (64 - eo.U_BITS) == m


def test_hash_broadcasts_like_the_kernel_rows():
    seeds = np.array([0, -1, 2 ** 63 - 1], dtype=np.int64)
    ctrs = np.array([0, 4095, 2 ** 31 - 1], dtype=np.int64)
    u = eo.row_noise(seeds, ctrs, 50)
    assert u.shape == (3, 50) and u.dtype == np.float32
    for r in range(3):
        for v in (0, 7, 49):
            assert float(u[r, v]) == _u01_int(int(seeds[r]), int(ctrs[r]),
                                              v, eo.U_BITS)[1]


@pytest.mark.parametrize("ctr,v,top", [
    (0, 5, (1 << 24) - 1), (4095, 4103, (1 << 24) - 1), (4095, 63, 0),
    (2 ** 31 - 1, 128255, 0xABCDEF), (1, 0, 1 << 23)])
def test_solve_seed_round_trips(ctr, v, top):
    seed = eo.solve_seed(ctr, v, top)
    assert -2 ** 63 <= seed < 2 ** 63
    assert int(eo.hash_key(seed, ctr, v)[0]) >> 40 == top
    assert _u01_int(seed, ctr, v, 24)[0] == top
    # and through another width
    s23 = eo.solve_seed(ctr, v, top >> 1, nbits=23)
    assert int(eo.hash_key(s23, ctr, v)[0]) >> 41 == top >> 1


def test_poison_seed_sets_all_top_bits():
    assert int(eo.hash_key(eo.POISON_SEED, eo.POISON_CTR,
                           eo.POISON_V)[0]) >> 40 == (1 << 24) - 1
    # under the parent's mapping that is u == 1 and infinite noise
    u_old = eo.hash_u01(eo.POISON_SEED, 0, 5, nbits=24)
    assert float(u_old[0]) == 1.0
    with np.errstate(divide="ignore"):
        assert np.isinf(-np.log(-np.log(u_old)))[0]
    u_new = eo.hash_u01(eo.POISON_SEED, 0, 5)
    assert float(u_new[0]) == 1.0 - 2.0 ** -24
    for V in eo.REGRESSION_V:
        _, seeds, ctrs = eo.regression_case(V, 1)
        assert int(eo.hash_key(int(seeds[1]), int(ctrs[1]), V - 1)[0]) \
            >> 40 == (1 << 24) - 1
        assert int(ctrs[1]) != 0


def test_uniform_mapping_is_strictly_inside_the_unit_interval():
    """Every mantissa the kernel can produce: u in (0, 1), strictly
    increasing, -log(-log(u)) finite in float32 at both ends (and
    everywhere).  The same enumeration of the parent's 24-bit mapping
    finds u == 1.0: the regression proof."""
    m = np.arange(1 << eo.U_BITS, dtype=np.uint64)
    u = eo.u01_of_mantissa(m)
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert float(u[0]) == 2.0 ** -(eo.U_BITS + 1)
    assert float(u[-1]) == 1.0 - 2.0 ** -(eo.U_BITS + 1)
    assert bool((np.diff(u) > 0).all())
    # exact: nothing was rounded
    assert bool((u.astype(np.float64) ==
                 (2.0 * m.astype(np.float64) + 1) * 2.0 ** -(eo.U_BITS + 1))
                .all())
    g = -np.log(-np.log(u))
    assert g.dtype == np.float32 and bool(np.isfinite(g).all())
    assert -2.83 < float(g[0]) < -2.81 and 16.6 < float(g[-1]) < 16.7
    # the parent: 24 bits + 0.5f is a tie above 2^23 and rounds up to 2^24
    m24 = np.arange(1 << 24, dtype=np.uint64)
    u24 = eo.u01_of_mantissa(m24, nbits=24)
    assert float(u24.max()) == 1.0
    assert int((u24 == 1.0).sum()) == 1 and float(u24[-1]) == 1.0
    assert not bool((np.diff(u24) > 0).all())


# ---------------------------------------------------------------------------
# budgets: an fp32 round-once emulation of each formula sits inside them


@pytest.mark.parametrize("H", eo.RMS_H)
def test_rmsnorm_emulation_inside_budget(H):
    worst = 0.0
    for T in eo.RMS_T:
        x, res, w = eo.rms_inputs(T, H)
        for r in (res, None):
            worst = max(worst, eo.assert_rows_close(
                eo.emulate_rmsnorm(x, r, w), eo.rmsnorm_oracle(x, r, w),
                f"rms H={H} T={T}"))
    for with_res in (False, True):
        x, res, w = eo.spike_inputs(H, with_res)
        assert x.shape[0] == len(eo.spike_positions(H))
        h = x.float() + (res.float() if with_res else 0)
        for r, p in enumerate(eo.spike_positions(H)):
            assert float(h[r, p]) == eo.SPIKE
            assert int((h[r].abs() == 1).sum()) == H - 1
        worst = max(worst, eo.assert_rows_close(
            eo.emulate_rmsnorm(x, res, w), eo.rmsnorm_oracle(x, res, w),
            f"spike H={H}"))
    print(f"[elem-oracle] rmsnorm H={H} emulation worst {worst:.3f}")


@pytest.mark.parametrize("H", (16, 2056, 8200, 16384))
def test_spike_rows_expose_a_dropped_vector(H):
    """Leave the spike's 16-byte vector out of the sum of squares, as a
    kernel with a wrong tail bound would: the budget must reject it."""
    x, res, w = eo.spike_inputs(H, False)
    truth = eo.rmsnorm_oracle(x, res, w)
    for r, p in enumerate(eo.spike_positions(H)):
        h = x[r:r + 1].float()
        keep = torch.ones(H)
        keep[p // 8 * 8:p // 8 * 8 + 8] = 0
        inv = torch.rsqrt((h * h * keep).sum() / H + eo.EPS)
        bad = (h * inv * w.float()).bfloat16()
        with pytest.raises(AssertionError):
            fo.assert_bf16_close(bad[0], truth[r])


def test_res_out_exact_is_one_rounding():
    x, res, _ = eo.rms_inputs(5, 512)
    want = (x.double() + res.double()).bfloat16()      # exact sum, one round
    assert torch.equal(eo.res_out_exact(x, res), want)
    assert eo.res_out_exact(x, None) is x


@pytest.mark.parametrize("Hq,Hk", eo.ROPE_HEADS)
def test_rope_emulation_inside_budget_and_exact_tier(Hq, Hk):
    cos, sin = fo.rope_tables(eo.ROPE_CTX)
    ccos, csin = eo.code_tables()
    assert set(ccos.unique().tolist()) == {-1.0, 0.0, 1.0}
    assert bool(((ccos.abs() + csin.abs()) == 1).all())
    assert bool((ccos[0] == 1).all()) and bool((csin[0] == 0).all())
    worst = 0.0
    for T in eo.ROPE_T:
        pos = eo.rope_positions(T)
        assert int(pos[0]) == eo.ROPE_CTX - 1 and (T == 1 or int(pos[1]) == 0)
        assert T == 1 or pos.tolist() != sorted(pos.tolist())
        q, k, _ = eo.rope_inputs(T, Hq, Hk)
        for t in (q, k):
            worst = max(worst, eo.assert_rows_close(
                eo.emulate_rope(t, pos, cos, sin),
                fo.rope_oracle(t.double(), pos, cos, sin), "rope"))
            # exact tier: the oracle's values are bf16 values already, and
            # the fp32 emulation reproduces them bit for bit
            ex = fo.rope_oracle(t.double(), pos, ccos, csin)
            assert torch.equal(ex.bfloat16().double(), ex)
            assert torch.equal(eo.emulate_rope(t, pos, ccos, csin),
                               ex.bfloat16())
            # a kernel that indexed the table by row instead of pos[t]
            wrong = fo.rope_oracle(t.double(), torch.arange(T), ccos, csin)
            assert not torch.equal(wrong, ex)
            one = torch.tensor([0])
            assert torch.equal(
                fo.rope_oracle(t[:1].double(), one, ccos, csin).bfloat16(),
                t[:1])
    print(f"[elem-oracle] rope ({Hq},{Hk}) emulation worst {worst:.3f}")


def test_rope_cases_leave_a_partial_block():
    assert any(T * (Hq + Hk) % 4 for T in eo.ROPE_T
               for Hq, Hk in eo.ROPE_HEADS)
    assert any(T * (Hq + 2 * Hk) % 4 for T in (3, 21)
               for Hq, Hk in eo.ROPE_HEADS)


@pytest.mark.parametrize("T,F", eo.SWIGLU_CASES)
def test_swiglu_emulation_inside_budget(T, F):
    gu = eo.swiglu_inputs(T, F)
    assert gu[0, :6].float().tolist() == [100, -100, 88, -88, 0, 0]
    worst = eo.assert_rows_close(eo.emulate_swiglu(gu),
                                 fo.swiglu_oracle(gu.double()),
                                 f"swiglu {T}x{F}")
    print(f"[elem-oracle] swiglu {T}x{F} emulation worst {worst:.3f}")


def test_loop_cases_exceed_one_grid_pass():
    T, F = eo.SWIGLU_CASES[-1]
    assert T * F // 8 > 2048 * 256
    assert 2049 * 8192 // 8 > 8192 * 256


# ---------------------------------------------------------------------------
# pools


@pytest.mark.parametrize("KVH", (1, 2, 3))
def test_append_pool_is_adversarial(KVH):
    pool = eo.append_pool(KVH, seed=KVH)
    c = pool.cache
    assert c.k_pool.shape[0] == ao.LAYERS == 3 and ao.LAYER == 1
    assert pool.slots != list(range(eo.APPEND_SEQS))
    for s in pool.slots:
        pages = c.page_table[s, :eo.APPEND_CAP // ao.PAGE].tolist()
        assert pages != sorted(pages) and len(set(pages)) == len(pages)
    for p in (c.k_pool, c.v_pool):
        assert bool(torch.isfinite(p.float()).all())
        assert bool((p != 0).all())
    rows = torch.cat([eo.bits(c.k_pool).reshape(-1, eo.D),
                      eo.bits(c.v_pool).reshape(-1, eo.D)])
    assert torch.unique(rows, dim=0).shape[0] == rows.shape[0]
    for kind, T in (("mixed", 21), ("decode", 3)):
        slots, pos = eo.append_batch(pool, kind)
        assert slots.shape == pos.shape == (T,)
        assert len(set(zip(slots.tolist(), pos.tolist()))) == T
        assert set(slots.tolist()) == set(pool.slots)
        if kind == "mixed":
            assert set(pos.tolist()) == set(eo.APPEND_POS)
            assert pos.tolist() != sorted(pos.tolist())
        else:
            assert len(set(pos.tolist())) == T
        src = fo.rand_bf16(T, KVH, eo.D, seed=5)
        after = eo.pool_after(c.k_pool, c.page_table, slots, pos, src)
        diff = (eo.bits(after) != eo.bits(c.k_pool)).reshape(
            ao.LAYERS, -1, KVH, ao.PAGE, eo.D).any(-1)
        assert int(diff.sum()) == T * KVH
        assert not bool(diff[0].any()) and not bool(diff[2].any())
        for t in range(T):
            pg = int(c.page_table[slots[t], pos[t] // ao.PAGE])
            assert torch.equal(after[1, pg, :, int(pos[t]) % ao.PAGE], src[t])


# ---------------------------------------------------------------------------
# argmax rows


@pytest.mark.parametrize("V", (eo.ARGMAX_V, eo.ARGMAX_BIG_V)
                         + eo.ARGMAX_SMALL_V + eo.ARGMAX_ODD_V)
def test_argmax_rows(V):
    pairs = eo.tie_pairs(V)
    assert (0, V - 1) in pairs
    if V > 2056:
        for need in ((8, 2056), (7, 8), (511, 512), (2047, 2048),
                     (2048, 4095)):
            assert need in pairs
    for m in range(2048, V, 2048):
        assert (m - 1, m) in pairs
        assert m + 2047 >= V or (m, m + 2047) in pairs
    rows, exp = eo.argmax_rows(V)
    assert rows.shape == (len(pairs) + 3, V)
    assert exp[:len(pairs)].tolist() == [a for a, _ in pairs]
    assert exp[len(pairs):].tolist() == [V - 1, 0, max(0, V - 3)]
    assert torch.equal(rows.float().bfloat16(), rows)
    for B in (1, 25, 769):
        seen = {i for b in eo.batches(rows.shape[0], B) for i in b}
        assert seen == set(range(rows.shape[0]))
        assert all(len(b) == B for b in eo.batches(rows.shape[0], B))


# ---------------------------------------------------------------------------
# the Gumbel decision margin


def test_gumbel_cases_cover_the_key_space():
    seeds, ctrs = set(), set()
    for B, V in eo.GUMBEL_CASES:
        logits, temps, sd, ct = eo.gumbel_case(B, V)
        assert logits.shape == (B, V) and logits.dtype == torch.bfloat16
        seeds |= set(sd.tolist())
        ctrs |= set(ct.tolist())
        if B >= 4:
            assert torch.equal(logits[0], logits[3])
            assert (int(sd[1]), int(ct[1])) == (int(sd[0]), int(ct[0]))
            assert int(sd[2]) != int(sd[0]) and int(ct[2]) == int(ct[0])
            assert int(sd[3]) == int(sd[0]) and int(ct[3]) != int(ct[0])
            u = eo.row_noise(sd[:4].numpy(), ct[:4].numpy(), V)
            assert (u[0] == u[1]).all()
            # a change of seed alone, or of ctr alone, redraws the noise
            assert (u[0] != u[2]).mean() > 0.99
            assert (u[0] != u[3]).mean() > 0.99
        if B >= 7:
            assert float(temps[5]) == 0.0 and float(temps[6]) == -1.0
            for r in (5, 6):
                top = logits[r].float()
                assert int((top == top.max()).sum()) == 2
    assert seeds == set(eo.SEED_POOL) and ctrs == set(eo.CTR_POOL)
    assert min(seeds) < 0 and max(seeds) == 2 ** 63 - 1


def test_gumbel_margin():
    """gamma = 16 x the largest |float32 emulation - fp64 score| over all
    cases; at most 2 % of the rows of any case may sit below it (a cap on
    how much of the test is allowed to be a two-way choice)."""
    worst = 0.0
    for B, V in eo.GUMBEL_CASES:
        logits, temps, sd, ct = eo.gumbel_case(B, V)
        best, runner, gap, err = eo.gumbel_expected(B, V)
        worst = max(worst, err)
        samp = temps.numpy() > 0
        assert bool((best != runner).all())
        assert bool((gap[samp] >= 0).all()) and bool(np.isinf(gap[~samp])
                                                     .all())
        below = int((gap < eo.GUMBEL_GAMMA).sum())
        print(f"[elem-oracle] gumbel {B}x{V}: f32 err {err:.3g}, "
              f"rows below gamma {below}/{B}, min gap {gap.min():.3g}")
        assert below <= 0.02 * B, (B, V, below)
        # greedy rows: the lowest index of the planted pair
        g = np.nonzero(~samp)[0]
        want = logits.float().numpy().argmax(axis=1)
        assert (best[g] == want[g]).all()
        # the sampled rows do sample: not the plain argmax everywhere
        if samp.sum() >= 4:
            assert (best[samp] != want[samp]).any()
    print(f"[elem-oracle] gumbel worst f32 err {worst:.4g}, "
          f"gamma {eo.GUMBEL_GAMMA:.4g}")
    assert eo.GUMBEL_GAMMA == 16 * eo.GUMBEL_F32_ERR
    assert eo.GUMBEL_F32_ERR / 2 <= worst <= eo.GUMBEL_F32_ERR, worst


def test_regression_rows_cannot_lose_with_finite_noise():
    for V in eo.REGRESSION_V:
        for which in (0, 1):
            logits, seeds, ctrs = eo.regression_case(V, which)
            u = eo.row_noise(seeds.numpy(), ctrs.numpy(), V)
            sc = eo.gumbel_scores(logits, np.ones(3), u)
            assert (sc.argmax(axis=1) == 0).all()
            # the parent's mapping picks the poisoned token in the middle
            u24 = eo.row_noise(seeds.numpy(), ctrs.numpy(), V, nbits=24)
            with np.errstate(divide="ignore"):
                old = eo.gumbel_scores(logits, np.ones(3), u24)
            assert old.argmax(axis=1).tolist() == \
                [0, eo.POISON_V if which == 0 else V - 1, 0]
