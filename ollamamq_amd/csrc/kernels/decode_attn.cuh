// Decode attention: the one definition of the per-segment KV sweep, the
// split-partial merge and the output store.  decode_attn.hip (one block per
// segment, partials through global memory) and decode_attn_blk.hip (all of
// a (sequence, kv-head)'s segments in one block, partials through LDS)
// both call these, so the two paths cannot disagree on the arithmetic.
#pragma once

#include "common.cuh"

#define DCHUNK 64
#define DHEAD 128
#define DKPAD 4
#define DKROW (DHEAD + DKPAD)

// bytes of one segment's K tile + V tile
constexpr int decode_tile_bytes(int CH) { return 2 * CH * DKROW * 2; }

// Segment bounds in whole chunks, balanced by floor interpolation (pages
// don't straddle chunks): ceil-div per_seg gave e.g. 9 chunks @ split 4 ->
// 3,3,3,0 with a whole workgroup idle; floor-interpolated bounds give
// 2,2,2,3.  Sliding window: the (single) query sits at kv_len-1, so only
// keys >= lo_tok participate; the ACTIVE chunk range is what is split.
struct DecodeRange { int lo_tok, ch_base, n_act; };

DEV DecodeRange decode_range(int kv_len, int window, int CH) {
    DecodeRange r;
    const int n_chunks = (kv_len + CH - 1) / CH;
    r.lo_tok = (window > 0 && kv_len > window) ? kv_len - window : 0;
    r.ch_base = r.lo_tok / CH;
    r.n_act = n_chunks - r.ch_base;
    return r;
}

DEV int decode_seg_bound(const DecodeRange& r, int seg, int split) {
    return r.ch_base + (int)(((int64_t)r.n_act * seg) / split);
}

// One segment's sweep over chunks [c0, c1): stage, score, online softmax,
// PV.  Run by the segment's GT waves (tid = 0 .. GT*64-1 within the
// segment, qrow/prow the calling wave's q and p rows) on the segment's own
// K/V tiles; (m, l, o0, o1) carry the wave's head, lane covering output
// dims (2*lane, 2*lane+1).
//
// Barriers are block-wide.  MULTI = false: the block IS the segment and
// runs c1 - c0 rounds.  MULTI = true: the block holds several segments and
// every one of them runs `n_rounds` (block-uniform, >= c1 - c0) rounds; a
// segment with no chunk left in a round issues no loads and does no
// arithmetic but still reaches both barriers.
template <int GT, int CH, bool MULTI>
DEV void decode_attn_segment(
    bf16* k_tile, bf16* v_tile, const float* qrow, float* prow,
    const bf16* __restrict__ kpool, const bf16* __restrict__ vpool,
    const int* __restrict__ page_table, int slot, int kv_len, int lo_tok,
    int kvh, int KVH, int page, int max_pages, float scale,
    int tid, int lane, int c0, int c1, int n_rounds,
    float& m, float& l, float& o0, float& o1)
{
    constexpr int NTHR = GT * 64;
    constexpr int KROW = DKROW;
    constexpr int NSLOT = CH * (DHEAD / 8);       // uint4 slots per tile
    constexpr int NPF = (NSLOT + NTHR - 1) / NTHR;  // prefetch regs/thread
    // Register-prefetch pipeline for every GQA group a preset uses.
    // Non-dividing groups (G=7, Qwen2: 1024 slots over 448 threads)
    // clamp the tail slot exactly like the prefill stager — duplicate
    // threads re-load/re-write identical bytes, which is benign, while a
    // guarded load/write would de-pipeline the stage (traps (c)).
    // NPF=8 (G=1 at chunk 32, G=2 at chunk 64) costs 64 VGPRs — free at
    // the 1-2 wave/SIMD occupancy LDS already imposes there.
    constexpr bool PF =
        (NPF <= 8) && (NSLOT % NTHR == 0 || NPF == 3);

    // clamp instead of guarding: a conditional load would de-pipeline the
    // whole stage (guide §5 traps (c)); the duplicated tail rows are
    // masked to p=0 by the softmax
    auto src_of = [&](int base, int u) -> int64_t {
        const int tok = u / (DHEAD / 8), dv = u % (DHEAD / 8);
        const int tk = base + tok < kv_len ? base + tok : kv_len - 1;
        return paged_kv_row(page_table, slot, max_pages, tk, page, KVH, kvh)
               + dv * 8;
    };
    auto stage_direct = [&](int ch2) {
        const int base2 = ch2 * CH;
        for (int u = tid; u < NSLOT; u += NTHR) {
            const int tok = u / (DHEAD / 8), dv = u % (DHEAD / 8);
            const int64_t src = src_of(base2, u);
            *reinterpret_cast<uint4*>(k_tile + tok * KROW + dv * 8) =
                *reinterpret_cast<const uint4*>(kpool + src);
            *reinterpret_cast<uint4*>(v_tile + tok * KROW + dv * 8) =
                *reinterpret_cast<const uint4*>(vpool + src);
        }
    };

    if (c0 < c1) stage_direct(c0);
    __syncthreads();

    if (!MULTI) n_rounds = c1 - c0;
    for (int r = 0; r < n_rounds; r++) {
        const int ch = c0 + r;
        const bool act = !MULTI || ch < c1;       // segment has this chunk
        const bool more = MULTI ? r + 1 < n_rounds : ch + 1 < c1;
        const int base = ch * CH;
        const int n_here = min(CH, kv_len - base);
        // ---- issue next chunk's HBM loads NOW, write to LDS after the
        // compute phase (T14 issue-early/write-late): the fetch rides
        // under the score/PV work instead of serializing with it.
        // Named registers, not an array — hipcc demotes even
        // constant-indexed uint4 arrays here to scratch (24 scratch ops,
        // 144 B/lane), and a spilled prefetch is HBM traffic, not a win.
        uint4 k0, k1, k2, k3, v0, v1, v2, v3;
        uint4 k4, k5, k6, k7, v4, v5, v6, v7;
        const bool have_next = PF && (ch + 1 < c1);
        if (have_next) {
            const int nbase = (ch + 1) * CH;
            const int64_t s0 = src_of(nbase, tid);
            const int64_t s1 = NPF >= 2 ? src_of(nbase, tid + NTHR) : s0;
            k0 = *reinterpret_cast<const uint4*>(kpool + s0);
            v0 = *reinterpret_cast<const uint4*>(vpool + s0);
            if constexpr (NPF >= 2) {
                k1 = *reinterpret_cast<const uint4*>(kpool + s1);
                v1 = *reinterpret_cast<const uint4*>(vpool + s1);
            }
            if constexpr (NPF >= 3) {
                const int64_t s2 = src_of(
                    nbase, min(tid + 2 * NTHR, NSLOT - 1));
                k2 = *reinterpret_cast<const uint4*>(kpool + s2);
                v2 = *reinterpret_cast<const uint4*>(vpool + s2);
            }
            if constexpr (NPF >= 4) {
                const int64_t s3 = src_of(nbase, tid + 3 * NTHR);
                k3 = *reinterpret_cast<const uint4*>(kpool + s3);
                v3 = *reinterpret_cast<const uint4*>(vpool + s3);
            }
            if constexpr (NPF >= 8) {
                const int64_t s4 = src_of(nbase, tid + 4 * NTHR);
                const int64_t s5 = src_of(nbase, tid + 5 * NTHR);
                const int64_t s6 = src_of(nbase, tid + 6 * NTHR);
                const int64_t s7 = src_of(nbase, tid + 7 * NTHR);
                k4 = *reinterpret_cast<const uint4*>(kpool + s4);
                v4 = *reinterpret_cast<const uint4*>(vpool + s4);
                k5 = *reinterpret_cast<const uint4*>(kpool + s5);
                v5 = *reinterpret_cast<const uint4*>(vpool + s5);
                k6 = *reinterpret_cast<const uint4*>(kpool + s6);
                v6 = *reinterpret_cast<const uint4*>(vpool + s6);
                k7 = *reinterpret_cast<const uint4*>(kpool + s7);
                v7 = *reinterpret_cast<const uint4*>(vpool + s7);
            }
        }

        if (act) {
            // ---- score for key j = lane ----
            float s = 0.f;
            const bool live = lane < n_here && base + lane >= lo_tok;
            {
                const bf16* krow = k_tile + lane * KROW;
                #pragma unroll
                for (int d = 0; d < DHEAD; d += 8) {
                    float k8[8];
                    load8f(krow + d, k8);
                    s += k8[0] * qrow[d] + k8[1] * qrow[d + 1]
                       + k8[2] * qrow[d + 2] + k8[3] * qrow[d + 3]
                       + k8[4] * qrow[d + 4] + k8[5] * qrow[d + 5]
                       + k8[6] * qrow[d + 6] + k8[7] * qrow[d + 7];
                }
                s = live ? s * scale : -3.0e38f;
            }

            // ---- online softmax ----
            const float smax = wave_reduce_max(s);
            float p = 0.f;
            if (smax > -3.0e38f) {
                const float mn = fmaxf(m, smax);
                const float corr = __expf(m - mn);
                p = live ? __expf(s - mn) : 0.f;
                l = l * corr + wave_reduce_sum(p);
                o0 *= corr; o1 *= corr;
                m = mn;
            }
            prow[lane] = p;

            // ---- PV: lane accumulates dims (2*lane, 2*lane+1) ----
            // fixed bound + full unroll: a runtime bound left this loop a
            // serial ds_read latency chain (PMC: 25% SQ_WAIT_INST_ANY);
            // dead keys contribute p=0 so looping to CH is exact
            #pragma unroll 8
            for (int j = 0; j < CH; j++) {
                const bf162 v2 = *reinterpret_cast<const bf162*>(
                    v_tile + j * KROW + 2 * lane);
                const float pj = prow[j];
                o0 = fmaf(pj, bf2f(v2.x), o0);
                o1 = fmaf(pj, bf2f(v2.y), o1);
            }
        }
        __syncthreads();  // every wave done reading the k/v tiles
        if (!more) continue;
        if (have_next) {
            auto put = [&](int u, uint4 kx, uint4 vx) {
                const int tok = u / (DHEAD / 8), dv = u % (DHEAD / 8);
                *reinterpret_cast<uint4*>(k_tile + tok * KROW + dv * 8)
                    = kx;
                *reinterpret_cast<uint4*>(v_tile + tok * KROW + dv * 8)
                    = vx;
            };
            put(tid, k0, v0);
            if constexpr (NPF >= 2) put(tid + NTHR, k1, v1);
            if constexpr (NPF >= 3)
                put(min(tid + 2 * NTHR, NSLOT - 1), k2, v2);
            if constexpr (NPF >= 4) put(tid + 3 * NTHR, k3, v3);
            if constexpr (NPF >= 8) {
                put(tid + 4 * NTHR, k4, v4);
                put(tid + 5 * NTHR, k5, v5);
                put(tid + 6 * NTHR, k6, v6);
                put(tid + 7 * NTHR, k7, v7);
            }
        } else if (!PF && ch + 1 < c1) {
            stage_direct(ch + 1);
        }
        __syncthreads();  // tiles ready for next iteration
    }
}

// Store one head's normalised output pair (dims 2*lane, 2*lane+1) of
// sequence S_idx: [S, Hq, D], or the fused-chain frag layout (fragout).
DEV void decode_store(bf16* __restrict__ out, int S_idx, int qh, int Hq,
                      int lane, int fragout, float a0, float a1) {
    const bf162 ov = __float22bfloat162_rn(make_float2(a0, a1));
    if (fragout)
        *reinterpret_cast<bf162*>(
            out + (int64_t)(S_idx >> 5) * 32 * Hq * DHEAD
                + frag_off(S_idx & 31, qh * DHEAD + 2 * lane)) = ov;
    else
        reinterpret_cast<bf162*>(
            out + ((int64_t)S_idx * Hq + qh) * DHEAD)[lane] = ov;
}

// Merge one head's `split` online-softmax partials exactly and store:
// m* = max m_i; o = Σ e^{m_i-m*} o_i; l = Σ e^{m_i-m*} l_i.  op is the
// head's [split][128] o partials, mlp its [split][2] (m, l) pairs, in
// global memory or LDS.  Run by one wave.
DEV void decode_merge_store(bf16* __restrict__ out, const float* op,
                            const float* mlp, int split, int S_idx, int qh,
                            int Hq, int lane, int fragout) {
    float m = -3.0e38f;
    for (int i = 0; i < split; i++)
        m = fmaxf(m, mlp[i * 2]);
    float l = 0.f, a0 = 0.f, a1 = 0.f;
    for (int i = 0; i < split; i++) {
        const float mi = mlp[i * 2];
        if (mi <= -3.0e38f) continue;
        const float w = __expf(mi - m);
        l += w * mlp[i * 2 + 1];
        a0 = fmaf(w, op[i * DHEAD + 2 * lane], a0);
        a1 = fmaf(w, op[i * DHEAD + 2 * lane + 1], a1);
    }
    const float linv = l > 0.f ? 1.f / l : 0.f;
    decode_store(out, S_idx, qh, Hq, lane, fragout, a0 * linv, a1 * linv);
}
