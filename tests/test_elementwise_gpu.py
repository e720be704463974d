"""k_rmsnorm_residual, k_rope, k_kv_append, k_rope_append, k_swiglu,
k_embed_gather and k_row_sumsq against the fp64 oracles of
tests/elem_oracle.py, through ollamamq_amd.ops.hip directly.

Real-valued outputs: |got - truth| <= 2^-7 |truth| + 2^-8 rms(truth) per
element, rms per row (fused_oracle.assert_bf16_close; an fp32 round-once
emulation of every formula sits inside it at every shape used here, see
test_elem_oracle_cpu.py).  Everything that is a copy, a single rounding of
an exact sum, a rotation by a +-1 / 0 table entry or an integer sum below
2^24 must be bit-equal.  The worst normalised error of each group is
printed (pytest -s) and recorded in docs/KERNELS.md.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_oracle as ao
import elem_oracle as eo
import fused_oracle as fo

DEV = "cuda:0"
APPEND_CTX = eo.APPEND_CAP      # rope table rows the append tests need


def _hip():
    from ollamamq_amd.ops import hip
    hip.require()
    return hip


def _g(t):
    """A fresh device copy (the kernels under test write in place)."""
    return t.to(DEV, copy=True)


def _report(group, worst):
    print(f"[elem-oracle] {group}: worst normalised error {worst:.3f}")


# ---------------------------------------------------------------------------
# rmsnorm + residual


@pytest.mark.parametrize("H", eo.RMS_H)
def test_rmsnorm_residual_oracle(H):
    hip = _hip()
    worst = 0.0
    for T in eo.RMS_T:
        x, res, w = eo.rms_inputs(T, H)
        for r in (res, None):
            y, ro = hip.rmsnorm_residual(
                _g(x), None if r is None else _g(r), _g(w),
                eo.EPS)
            assert torch.equal(ro.cpu(), eo.res_out_exact(x, r)), \
                f"res_out H={H} T={T} res={r is not None}"
            worst = max(worst, eo.assert_rows_close(
                y, eo.rmsnorm_oracle(x, r, w),
                f"rmsnorm H={H} T={T} res={r is not None}"))
    _report(f"rmsnorm_residual H={H}", worst)


@pytest.mark.parametrize("H", eo.RMS_H)
def test_rmsnorm_residual_spike_rows(H):
    """+-1 rows with one element of 64 at 0, 7, 8, 2047, 2048, H-8, H-1:
    the vector holding it dropped from the reduction moves rstd by 1.29x
    at H = 16384, 2.0x at H = 2048 and more below, against one bf16 ulp."""
    hip = _hip()
    worst = 0.0
    for with_res in (False, True):
        x, res, w = eo.spike_inputs(H, with_res)
        y, ro = hip.rmsnorm_residual(
            _g(x), _g(res) if with_res else None, _g(w), eo.EPS)
        assert torch.equal(ro.cpu(), eo.res_out_exact(x, res))
        worst = max(worst, eo.assert_rows_close(
            y, eo.rmsnorm_oracle(x, res, w), f"spike H={H} res={with_res}"))
    _report(f"rmsnorm_residual spikes H={H}", worst)


def test_rmsnorm_residual_rejects_what_the_kernel_cannot_do():
    hip = _hip()
    w = torch.ones(16392, dtype=torch.bfloat16, device=DEV)
    x = torch.ones(2, 16392, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(ValueError):
        hip.rmsnorm_residual(x, None, w, eo.EPS)            # H > 16384
    with pytest.raises(ValueError):
        hip.rmsnorm_residual(x[:, :12], None, w[:12], eo.EPS)   # H % 8
    wide = torch.ones(4, 1024, dtype=torch.bfloat16, device=DEV)
    ok = torch.ones(4, 512, dtype=torch.bfloat16, device=DEV)
    assert not wide[:, :512].is_contiguous()
    with pytest.raises(ValueError):
        hip.rmsnorm_residual(wide[:, :512], ok, w[:512], eo.EPS)
    with pytest.raises(ValueError):
        hip.rmsnorm_residual(ok, wide[:, 512:], w[:512], eo.EPS)
    with pytest.raises(ValueError):
        hip.rmsnorm_residual(ok, None, w[:1024:2], eo.EPS)
    # the launcher itself refuses the size as well
    y, ro = torch.empty_like(x), torch.empty_like(x)
    err = hip._lib.rmsnorm_residual_bf16(
        hip._p(y), hip._p(ro), hip._p(x), hip._p(None), hip._p(w), 2, 16392,
        eo.EPS, hip._stream())
    assert err == 1, err                       # hipErrorInvalidValue
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# rope


def _rope_check(hip, T, Hq, Hk, cos, sin, fused, exact):
    """Run hip.rope on q, k (contiguous, or views of a fused buffer whose v
    columns are NaN) and hold both to the oracle."""
    pos = eo.rope_positions(T)
    q, k, _ = eo.rope_inputs(T, Hq, Hk)
    if fused:
        buf, qg, kg, vg = eo.fused_views(_g(q), _g(k))
        assert T == 1 or not qg.is_contiguous()
        before = eo.bits(vg)
    else:
        qg, kg = _g(q), _g(k)
    hip.rope(qg, kg, _g(pos), _g(cos), _g(sin))
    worst = 0.0
    for got, src, name in ((qg, q, "q"), (kg, k, "k")):
        truth = fo.rope_oracle(src.double(), pos, cos, sin)
        tag = f"rope {name} T={T} ({Hq},{Hk}) fused={fused}"
        if exact:
            assert torch.equal(got.cpu(), truth.bfloat16()), tag
        else:
            worst = max(worst, eo.assert_rows_close(got, truth, tag))
    if fused:
        assert torch.equal(eo.bits(vg), before), "rope touched the v columns"
    return worst


@pytest.mark.parametrize("Hq,Hk", eo.ROPE_HEADS)
def test_rope_exact_codes(Hq, Hk):
    """cos/sin in {(1,0), (0,1), (-1,0), (0,-1)} per (position, lane):
    every output is +-x1 or +-x2, bit for bit; catches t for pos[t], a wrong
    lane and a wrong table stride."""
    hip = _hip()
    cos, sin = eo.code_tables()
    for T in eo.ROPE_T:
        for fused in (False, True):
            _rope_check(hip, T, Hq, Hk, cos, sin, fused, exact=True)
    # position 0 is the identity
    q, k, _ = eo.rope_inputs(5, Hq, Hk, seed=1)
    qg, kg = _g(q), _g(k)
    zero = torch.zeros(5, dtype=torch.int32, device=DEV)
    for c, s in ((cos, sin), fo.rope_tables(eo.ROPE_CTX)):
        hip.rope(qg, kg, zero, _g(c), _g(s))
        assert torch.equal(qg.cpu(), q) and torch.equal(kg.cpu(), k)


@pytest.mark.parametrize("Hq,Hk", eo.ROPE_HEADS)
def test_rope_real(Hq, Hk):
    hip = _hip()
    cos, sin = fo.rope_tables(eo.ROPE_CTX)
    worst = 0.0
    for T in eo.ROPE_T:
        for fused in (False, True):
            worst = max(worst, _rope_check(hip, T, Hq, Hk, cos, sin, fused,
                                           exact=False))
    _report(f"rope ({Hq},{Hk})", worst)


# ---------------------------------------------------------------------------
# kv_append / rope_append on the adversarial pool


def _assert_pool(got, want, what):
    g, w = eo.bits(got), eo.bits(want)
    if not torch.equal(g, w):
        bad = (g != w).reshape(ao.LAYERS, -1, got.shape[2], ao.PAGE,
                               eo.D).any(-1).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} pool rows differ, "
                             f"first (layer, page, head, offset) "
                             f"{bad[0].tolist()}")


@pytest.mark.parametrize("kind", ("mixed", "decode"))
@pytest.mark.parametrize("Hq,KVH", eo.ROPE_HEADS)
def test_kv_append_adversarial_pool(Hq, KVH, kind):
    """Addressed rows bit-equal to the source (contiguous and strided),
    every other pool element of every layer bit-identical to its
    pre-fill."""
    hip = _hip()
    pool = eo.append_pool(KVH, seed=KVH)
    slots, pos = eo.append_batch(pool, kind, seed=Hq)
    T = pos.shape[0]
    q, k, v = eo.rope_inputs(T, Hq, KVH, seed=2)
    c = pool.cache
    want_k = eo.pool_after(c.k_pool, c.page_table, slots, pos, k)
    want_v = eo.pool_after(c.v_pool, c.page_table, slots, pos, v)
    for fused in (False, True):
        g = pool.to(DEV).cache
        if fused:
            _, _, kg, vg = eo.fused_views(_g(q), _g(k), _g(v))
            assert T == 1 or not kg.is_contiguous()
        else:
            kg, vg = _g(k), _g(v)
        hip.kv_append(g, ao.LAYER, kg, vg, _g(slots), _g(pos))
        _assert_pool(g.k_pool, want_k, f"k pool fused={fused}")
        _assert_pool(g.v_pool, want_v, f"v pool fused={fused}")
        assert torch.equal(kg.cpu(), k) and torch.equal(vg.cpu(), v)
        assert torch.equal(g.page_table.cpu(), c.page_table)


@pytest.mark.parametrize("kind", ("mixed", "decode"))
@pytest.mark.parametrize("Hq,KVH", eo.ROPE_HEADS)
def test_rope_append_adversarial_pool(Hq, KVH, kind):
    """q and k rotated in place (exact code tables: bit-equal; real tables:
    the fp64 budget), the pool's k rows bit-equal to the rotated k the same
    call returned, its v rows to the source, the rest of both pools
    untouched.  Contiguous inputs and fused-QKV views."""
    hip = _hip()
    pool = eo.append_pool(KVH, seed=10 + KVH)
    slots, pos = eo.append_batch(pool, kind, seed=Hq + 1)
    T = pos.shape[0]
    q, k, v = eo.rope_inputs(T, Hq, KVH, seed=3)
    c = pool.cache
    want_v = eo.pool_after(c.v_pool, c.page_table, slots, pos, v)
    worst = 0.0
    for exact in (True, False):
        cos, sin = eo.code_tables(APPEND_CTX) if exact \
            else fo.rope_tables(APPEND_CTX)
        tq = fo.rope_oracle(q.double(), pos, cos, sin)
        tk = fo.rope_oracle(k.double(), pos, cos, sin)
        for fused in (False, True):
            g = pool.to(DEV).cache
            if fused:
                _, qg, kg, vg = eo.fused_views(_g(q), _g(k),
                                               _g(v))
            else:
                qg, kg, vg = _g(q), _g(k), _g(v)
            hip.rope_append(g, ao.LAYER, qg, kg, vg, _g(pos),
                            _g(slots), _g(cos), _g(sin))
            tag = f"rope_append exact={exact} fused={fused}"
            if exact:
                assert torch.equal(qg.cpu(), tq.bfloat16()), tag
                assert torch.equal(kg.cpu(), tk.bfloat16()), tag
            else:
                worst = max(worst,
                            eo.assert_rows_close(qg, tq, tag + " q"),
                            eo.assert_rows_close(kg, tk, tag + " k"))
            assert torch.equal(vg.cpu(), v), tag
            _assert_pool(g.k_pool, eo.pool_after(
                c.k_pool, c.page_table, slots, pos, kg.cpu()), tag + " k pool")
            _assert_pool(g.v_pool, want_v, tag + " v pool")
    _report(f"rope_append ({Hq},{KVH}) {kind}", worst)



# ---------------------------------------------------------------------------
# swiglu


@pytest.mark.parametrize("T,F", eo.SWIGLU_CASES)
def test_swiglu_oracle(T, F):
    hip = _hip()
    gu = eo.swiglu_inputs(T, F)
    out = hip.swiglu(_g(gu))
    assert out.shape == (T, F)
    worst = eo.assert_rows_close(out, fo.swiglu_oracle(gu.double()),
                                 f"swiglu {T}x{F}")
    _report(f"swiglu {T}x{F}", worst)


def test_swiglu_rejects_a_vector_tail():
    hip = _hip()
    for F in (4, 12, 1028):
        gu = torch.zeros(3, 2 * F, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(ValueError):
            hip.swiglu(gu)


# ---------------------------------------------------------------------------
# embedding


def _ids(T, V, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (T,), generator=g)
    ids[0], ids[-1] = V - 1, 0
    if T > 4:
        ids[1] = ids[2] = ids[T // 2] = 0            # repeats
        ids[3] = V - 1
    return ids


def test_embedding_second_grid_pass():
    """2049 x 8192: 2 098 176 16-byte vectors, more than the 8192 x 256
    threads of the launch, so the grid-stride loop runs again."""
    hip = _hip()
    T, V, H = 2049, 64, 8192
    table = _g(fo.rand_bf16(V, H, seed=V + H))
    ids = _ids(T, V, 1)
    want = table.cpu()[ids]
    for dt in (torch.int64, torch.int32):
        out = hip.embedding(_g(ids.to(dt)), table)
        assert torch.equal(out.cpu(), want), dt


@pytest.mark.parametrize("T,V,H", [(1, 3, 8), (7, 1000, 3584), (33, 5, 12),
                                   (5, 9, 4)])
def test_embedding_small_and_fallback(T, V, H):
    """H % 8 != 0 takes the index_select fallback; both must be exact."""
    hip = _hip()
    table = _g(fo.rand_bf16(V, H, seed=V + H))
    ids = _ids(T, V, 2)
    want = table.cpu()[ids]
    for dt in (torch.int64, torch.int32):
        out = hip.embedding(_g(ids.to(dt)), table)
        assert out.dtype == torch.bfloat16 and torch.equal(out.cpu(), want)


# ---------------------------------------------------------------------------
# row_sumsq


@pytest.mark.parametrize("H", eo.SUMSQ_H)
def test_row_sumsq(H):
    hip = _hip()
    worst = 0.0
    for M in eo.SUMSQ_M:
        t = fo.ternary(M, H, seed=H + M)
        got = hip.row_sumsq(_g(t))
        assert got.dtype == torch.float32
        assert torch.equal(got.cpu().double(), t.double().pow(2).sum(1)), \
            f"ternary M={M} H={H}"
        x = fo.rand_bf16(M, H, seed=H + M + 1)
        worst = max(worst, fo.assert_sq_close(
            hip.row_sumsq(_g(x)), x.double().pow(2).sum(1),
            f"row_sumsq M={M} H={H}"))
    _report(f"row_sumsq H={H}", worst)
