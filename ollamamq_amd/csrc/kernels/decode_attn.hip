// gfx950 decode attention with KV-length splitting (flash-decoding style).
//
// Problem shape: B sequences × Hq heads × 1 query token, paged KV pool,
// GQA group G = Hq/KVH.  Memory-bound: the whole job is streaming each
// sequence's K+V (seq_len × 512 B per kv-head) once.  A (seq, kv-head)
// grid alone gives B×KVH blocks (256 at B=32 ⇒ 1 workgroup/CU, far too
// few to hide HBM latency — measured 0.65 TB/s).  Splitting the KV length
// into SPLIT segments multiplies parallelism: each block computes a
// partial (o, m, l) over its segment; a small combine kernel merges the
// online-softmax partials exactly.
//
// LDS: K/V chunk tiles shared by the group's G waves (each KV byte read
// once per kv-head, not per q-head); rows padded +4 bf16 to keep per-lane
// row reads conflict-free (guide §6 G4).
//
// fragout: the attention OUTPUT is written in the fused-chain frag layout
// (common.cuh frag_off) so the o-GEMM streams it linearly.
#include "common.cuh"

#define DCHUNK 64
#define DHEAD 128
#define DKPAD 4

// grid: (n_seqs * split, KVH); block: G*64 threads (G templated: the
// next-chunk register-prefetch array must be compile-time sized, guide
// rule 20 — runtime-indexed arrays land in scratch).
// Partials: o_part [S][Hq][split][128] f32, ml_part [S][Hq][split][2] f32.
// When split == 1, writes normalized bf16 straight to out.
// launch_bounds min-waves/EU = 1: LDS (~37 KB/block) already caps
// residency at 4 blocks/CU, so a high compiler occupancy target only
// forces the prefetch registers to spill (measured 144 B/lane scratch)
template <int GT, int CH>
__global__ __launch_bounds__(GT * 64, 1) void k_decode_attn(
    bf16* __restrict__ out,               // [S, Hq, D] (split==1)
    float* __restrict__ o_part,           // split>1 partials
    float* __restrict__ ml_part,
    const bf16* __restrict__ q,           // [S, Hq, D] (row stride qs)
    const bf16* __restrict__ kpool,       // [P][KVH][page][D]
    const bf16* __restrict__ vpool,
    const int* __restrict__ page_table,   // [slots][max_pages]
    const int* __restrict__ slot_ids,     // [S]
    const int* __restrict__ seq_lens,     // [S] (kv length incl. this tok)
    int Hq, int KVH, int page, int max_pages, float scale,
    int64_t qs, int split, int window,    // window 0 = full causal
    unsigned* __restrict__ sem,           // [S*KVH] tickets (fused combine)
    int fragout)                          // out in fused-chain frag layout
{
    const int S_idx = blockIdx.x / split;
    const int seg = blockIdx.x % split;
    const int kvh = blockIdx.y;
    constexpr int G = GT;
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int qh = kvh * G + wid;

    constexpr int NTHR = GT * 64;
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

    const int slot = slot_ids[S_idx];
    const int kv_len = seq_lens[S_idx];
    // balanced segment bounds in whole chunks (pages don't straddle
    // chunks): ceil-div per_seg gave e.g. 9 chunks @ split 4 -> 3,3,3,0
    // with a whole workgroup idle; floor-interpolated bounds give 2,2,2,3
    const int n_chunks = (kv_len + CH - 1) / CH;
    // sliding window: the (single) query sits at kv_len-1, so only keys
    // >= lo_tok participate; split the ACTIVE chunk range
    const int lo_tok = (window > 0 && kv_len > window) ? kv_len - window : 0;
    const int ch_base = lo_tok / CH;
    const int n_act = n_chunks - ch_base;
    const int c0 = ch_base + (int)(((int64_t)n_act * seg) / split);
    const int c1 = ch_base + (int)(((int64_t)n_act * (seg + 1)) / split);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int KROW = DHEAD + DKPAD;
    bf16* k_tile = reinterpret_cast<bf16*>(smem);
    bf16* v_tile = k_tile + CH * KROW;
    float* q_lds = reinterpret_cast<float*>(v_tile + CH * KROW); // [G][128]
    // p row is per-LANE (65 = 64+pad), NOT per-chunk-key: every lane
    // stores its p (dead lanes 0.0), so a CH=32 row of 33 floats would
    // send lanes 32-63 past the row (OOB at G=1, cross-wave race at G>1)
    float* p_lds = q_lds + (int64_t)G * DHEAD;                       // [G][65]

    // stage q (fp32 in LDS: repeated broadcast reads in the score loop)
    if (wid < G) {
        const bf16* qsrc = q + (int64_t)S_idx * qs + (int64_t)qh * DHEAD;
        q_lds[wid * DHEAD + lane] = bf2f(qsrc[lane]);
        q_lds[wid * DHEAD + lane + 64] = bf2f(qsrc[lane + 64]);
    }
    __syncthreads();

    float m = -3.0e38f, l = 0.f, o0 = 0.f, o1 = 0.f;

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
        for (int u = threadIdx.x; u < NSLOT; u += NTHR) {
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

    for (int ch = c0; ch < c1; ch++) {
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
            const int64_t s0 = src_of(nbase, threadIdx.x);
            const int64_t s1 = NPF >= 2 ? src_of(nbase, threadIdx.x + NTHR)
                                        : s0;
            k0 = *reinterpret_cast<const uint4*>(kpool + s0);
            v0 = *reinterpret_cast<const uint4*>(vpool + s0);
            if constexpr (NPF >= 2) {
                k1 = *reinterpret_cast<const uint4*>(kpool + s1);
                v1 = *reinterpret_cast<const uint4*>(vpool + s1);
            }
            if constexpr (NPF >= 3) {
                const int64_t s2 = src_of(
                    nbase, min((int)threadIdx.x + 2 * NTHR, NSLOT - 1));
                k2 = *reinterpret_cast<const uint4*>(kpool + s2);
                v2 = *reinterpret_cast<const uint4*>(vpool + s2);
            }
            if constexpr (NPF >= 4) {
                const int64_t s3 = src_of(nbase, threadIdx.x + 3 * NTHR);
                k3 = *reinterpret_cast<const uint4*>(kpool + s3);
                v3 = *reinterpret_cast<const uint4*>(vpool + s3);
            }
            if constexpr (NPF >= 8) {
                const int64_t s4 = src_of(nbase, threadIdx.x + 4 * NTHR);
                const int64_t s5 = src_of(nbase, threadIdx.x + 5 * NTHR);
                const int64_t s6 = src_of(nbase, threadIdx.x + 6 * NTHR);
                const int64_t s7 = src_of(nbase, threadIdx.x + 7 * NTHR);
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

        // ---- score for key j = lane ----
        float s = 0.f;
        const bool live = lane < n_here && base + lane >= lo_tok;
        {
            const bf16* krow = k_tile + lane * KROW;
            const float* qrow = q_lds + wid * DHEAD;
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
        p_lds[wid * 65 + lane] = p;

        // ---- PV: lane accumulates dims (2*lane, 2*lane+1) ----
        // fixed bound + full unroll: a runtime bound left this loop a
        // serial ds_read latency chain (PMC: 25% SQ_WAIT_INST_ANY);
        // dead keys contribute p=0 so looping to CH is exact
        const float* prow = p_lds + wid * 65;
        #pragma unroll 8
        for (int j = 0; j < CH; j++) {
            const bf162 v2 = *reinterpret_cast<const bf162*>(
                v_tile + j * KROW + 2 * lane);
            const float pj = prow[j];
            o0 = fmaf(pj, bf2f(v2.x), o0);
            o1 = fmaf(pj, bf2f(v2.y), o1);
        }
        __syncthreads();  // every wave done reading the k/v tiles
        if (have_next) {
            auto put = [&](int u, uint4 kx, uint4 vx) {
                const int tok = u / (DHEAD / 8), dv = u % (DHEAD / 8);
                *reinterpret_cast<uint4*>(k_tile + tok * KROW + dv * 8)
                    = kx;
                *reinterpret_cast<uint4*>(v_tile + tok * KROW + dv * 8)
                    = vx;
            };
            put(threadIdx.x, k0, v0);
            if constexpr (NPF >= 2) put(threadIdx.x + NTHR, k1, v1);
            if constexpr (NPF >= 3)
                put(min((int)threadIdx.x + 2 * NTHR, NSLOT - 1), k2, v2);
            if constexpr (NPF >= 4) put(threadIdx.x + 3 * NTHR, k3, v3);
            if constexpr (NPF >= 8) {
                put(threadIdx.x + 4 * NTHR, k4, v4);
                put(threadIdx.x + 5 * NTHR, k5, v5);
                put(threadIdx.x + 6 * NTHR, k6, v6);
                put(threadIdx.x + 7 * NTHR, k7, v7);
            }
            __syncthreads();  // tiles ready for next iteration
        } else if (!PF && ch + 1 < c1) {
            stage_direct(ch + 1);
            __syncthreads();
        }
    }

    // ---- emit ----
    if (split == 1) {
        const float linv = l > 0.f ? 1.f / l : 0.f;
        const bf162 ov =
            __float22bfloat162_rn(make_float2(o0 * linv, o1 * linv));
        if (fragout)
            *reinterpret_cast<bf162*>(
                out + (int64_t)(S_idx >> 5) * 32 * Hq * DHEAD
                    + frag_off(S_idx & 31, qh * DHEAD + 2 * lane))
                = ov;
        else
            reinterpret_cast<bf162*>(
                out + ((int64_t)S_idx * Hq + qh) * DHEAD)[lane] = ov;
        return;
    }
    {
        const int64_t pi = (((int64_t)S_idx * Hq + qh) * split + seg);
        float* op = o_part + pi * DHEAD;
        op[2 * lane] = o0;
        op[2 * lane + 1] = o1;
        ml_part[pi * 2] = m;
        ml_part[pi * 2 + 1] = l;
    }
    if (sem == nullptr) return;   // separate k_decode_combine pass (A/B)

    // ---- in-launch combine (guide §6 G16 split-K recipe): publish the
    // partials with an agent-scope release BEFORE the ticket fetch_add;
    // the block that draws split-1 acquires and reduces its (seq, kvh)
    // group — saves the combine kernel's launch boundary + HBM round trip
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();              // all waves' partials issued
    int* flag = reinterpret_cast<int*>(smem);   // tiles are dead; reuse
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        // restate the post-wbl2 wait the compiler may drop (pitfall 12)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(
            &sem[(int64_t)S_idx * gridDim.y + kvh], 1u,
            __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = (t == (unsigned)(split - 1)) ? 1 : 0;
    }
    __syncthreads();
    if (*flag == 0) return;
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // reset for the next launch (stream-ordered; all arrivals done)
        __hip_atomic_store(&sem[(int64_t)S_idx * gridDim.y + kvh], 0u,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();              // acquire visible to the whole block
    {
        // wave `wid` reduces its head, lane covers dims (2*lane, 2*lane+1)
        const int64_t sh = (int64_t)S_idx * Hq + qh;
        float mm = -3.0e38f;
        for (int i = 0; i < split; i++)
            mm = fmaxf(mm, ml_part[(sh * split + i) * 2]);
        float ll = 0.f, a0 = 0.f, a1 = 0.f;
        for (int i = 0; i < split; i++) {
            const int64_t pi = sh * split + i;
            const float mi = ml_part[pi * 2];
            if (mi <= -3.0e38f) continue;
            const float w = __expf(mi - mm);
            ll += w * ml_part[pi * 2 + 1];
            const float* op = o_part + pi * DHEAD;
            a0 = fmaf(w, op[2 * lane], a0);
            a1 = fmaf(w, op[2 * lane + 1], a1);
        }
        const float linv = ll > 0.f ? 1.f / ll : 0.f;
        if (fragout) {
            *reinterpret_cast<bf162*>(
                out + (int64_t)(S_idx >> 5) * 32 * Hq * DHEAD
                    + frag_off(S_idx & 31, qh * DHEAD + 2 * lane)) =
                __float22bfloat162_rn(
                    make_float2(a0 * linv, a1 * linv));
            return;
        }
        reinterpret_cast<bf162*>(out + sh * DHEAD)[lane] =
            __float22bfloat162_rn(make_float2(a0 * linv, a1 * linv));
    }
}

// combine: one wave per (seq, head); merges the split online-softmax
// partials exactly: m* = max m_i; o = Σ e^{m_i-m*} o_i; l = Σ e^{m_i-m*} l_i
__global__ __launch_bounds__(256) void k_decode_combine(
    bf16* __restrict__ out, const float* __restrict__ o_part,
    const float* __restrict__ ml_part, int total, int split,
    int Hq, int fragout)
{
    const int sh = blockIdx.x * 4 + (threadIdx.x >> 6);  // seq*Hq + head
    const int lane = threadIdx.x & 63;
    if (sh >= total) return;
    float m = -3.0e38f;
    for (int i = 0; i < split; i++)
        m = fmaxf(m, ml_part[((int64_t)sh * split + i) * 2]);
    float l = 0.f, a0 = 0.f, a1 = 0.f;
    for (int i = 0; i < split; i++) {
        const int64_t pi = (int64_t)sh * split + i;
        const float mi = ml_part[pi * 2];
        if (mi <= -3.0e38f) continue;
        const float w = __expf(mi - m);
        l += w * ml_part[pi * 2 + 1];
        const float* op = o_part + pi * DHEAD;
        a0 = fmaf(w, op[2 * lane], a0);
        a1 = fmaf(w, op[2 * lane + 1], a1);
    }
    const float linv = l > 0.f ? 1.f / l : 0.f;
    const bf162 ov =
        __float22bfloat162_rn(make_float2(a0 * linv, a1 * linv));
    if (fragout)
        *reinterpret_cast<bf162*>(
            out + (int64_t)((sh / Hq) >> 5) * 32 * Hq * DHEAD
                + frag_off((sh / Hq) & 31,
                           (sh % Hq) * DHEAD + 2 * lane)) = ov;
    else
        reinterpret_cast<bf162*>(out + (int64_t)sh * DHEAD)[lane] = ov;
}

extern "C" int decode_attn_bf16(
    void* out, void* o_part, void* ml_part, const void* q,
    const void* kpool, const void* vpool, const void* page_table,
    const void* slot_ids, const void* seq_lens, int S, int Hq, int KVH,
    int page, int max_pages, float scale, int64_t q_stride, int split,
    int window, int chunk, void* sem, int fragout, hipStream_t stream)
{
    const int G = Hq / KVH;
    const int lds = 2 * chunk * (DHEAD + DKPAD) * 2 + G * DHEAD * 4
                  + G * 65 * 4;
    dim3 grid(S * split, KVH);
#define DA_LAUNCH1(GT, CH)                                                \
    k_decode_attn<GT, CH><<<grid, GT * 64, lds, stream>>>(                \
        (bf16*)out, (float*)o_part, (float*)ml_part, (const bf16*)q,      \
        (const bf16*)kpool, (const bf16*)vpool, (const int*)page_table,   \
        (const int*)slot_ids, (const int*)seq_lens, Hq, KVH, page,        \
        max_pages, scale, q_stride, split, window, (unsigned*)sem,     \
        fragout)
// chunk is capped at 64: the score phase assigns ONE key per lane of a
// wave64, so a larger staged chunk would silently drop keys 64+ (a 128
// arm measured wrong before this guard)
#define DA_LAUNCH(GT)                                                     \
    switch (chunk) {                                                      \
        case 32: DA_LAUNCH1(GT, 32); break;                               \
        default: DA_LAUNCH1(GT, 64); break;                               \
    }
    switch (G) {
        case 1: DA_LAUNCH(1); break;
        case 2: DA_LAUNCH(2); break;
        case 3: DA_LAUNCH(3); break;
        case 4: DA_LAUNCH(4); break;
        case 5: DA_LAUNCH(5); break;
        case 6: DA_LAUNCH(6); break;
        case 7: DA_LAUNCH(7); break;
        case 8: DA_LAUNCH(8); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef DA_LAUNCH
#undef DA_LAUNCH1
    if (split > 1 && sem == nullptr) {
        const int waves = S * Hq;
        k_decode_combine<<<(waves + 3) / 4, 256, 0, stream>>>(
            (bf16*)out, (const float*)o_part, (const float*)ml_part, waves,
            split, Hq, fragout);
    }
    return (int)hipGetLastError();
}

// Pure-stage diagnostic: identical grid/segmentation/addressing to
// k_decode_attn but ONLY the KV loads (no LDS, no score/PV, no
// barriers) — the staging stream ceiling of this geometry.  If this
// matches the real kernel's time, the kernel is geometry/bandwidth
// capped and compute-side pipelining cannot help.
__global__ __launch_bounds__(256) void k_decode_pure(
    float* __restrict__ sink, const bf16* __restrict__ kpool,
    const bf16* __restrict__ vpool, const int* __restrict__ page_table,
    const int* __restrict__ slot_ids, const int* __restrict__ seq_lens,
    int KVH, int page, int max_pages, int split, int chunk)
{
    const int S_idx = blockIdx.x / split;
    const int seg = blockIdx.x % split;
    const int kvh = blockIdx.y;
    const int slot = slot_ids[S_idx];
    const int kv_len = seq_lens[S_idx];
    const int n_chunks = (kv_len + chunk - 1) / chunk;
    const int c0 = (int)(((int64_t)n_chunks * seg) / split);
    const int c1 = (int)(((int64_t)n_chunks * (seg + 1)) / split);
    const int nslot = chunk * 16;
    unsigned acc = 0;
    for (int ch = c0; ch < c1; ch++) {
        const int base = ch * chunk;
        for (int u = threadIdx.x; u < nslot; u += 256) {
            const int tok = u >> 4, dv = u & 15;
            const int tk = base + tok < kv_len ? base + tok : kv_len - 1;
            const int64_t src = paged_kv_row(page_table, slot, max_pages, tk,
                                             page, KVH, kvh) + dv * 8;
            const uint4 k = *reinterpret_cast<const uint4*>(kpool + src);
            const uint4 v = *reinterpret_cast<const uint4*>(vpool + src);
            acc ^= k.x ^ k.w ^ v.x ^ v.w;
        }
    }
    if (acc == 0xDEADBEEFu) sink[0] = 1.f;
}

extern "C" int decode_pure_bf16(
    void* sink, const void* kpool, const void* vpool,
    const void* page_table, const void* slot_ids, const void* seq_lens,
    int S, int KVH, int page, int max_pages, int split, int chunk,
    hipStream_t stream)
{
    dim3 grid(S * split, KVH);
    k_decode_pure<<<grid, 256, 0, stream>>>(
        (float*)sink, (const bf16*)kpool, (const bf16*)vpool,
        (const int*)page_table, (const int*)slot_ids,
        (const int*)seq_lens, KVH, page, max_pages, split, chunk);
    return (int)hipGetLastError();
}
