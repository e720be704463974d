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
//
// The segment sweep, the partial merge and the output store are defined
// once in decode_attn.cuh; decode_attn_blk.hip is the second caller.
#include "decode_attn.cuh"

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

    const int slot = slot_ids[S_idx];
    const int kv_len = seq_lens[S_idx];
    const DecodeRange rg = decode_range(kv_len, window, CH);
    const int c0 = decode_seg_bound(rg, seg, split);
    const int c1 = decode_seg_bound(rg, seg + 1, split);

    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* k_tile = reinterpret_cast<bf16*>(smem);
    bf16* v_tile = k_tile + CH * DKROW;
    float* q_lds = reinterpret_cast<float*>(v_tile + CH * DKROW); // [G][128]
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
    decode_attn_segment<GT, CH, false>(
        k_tile, v_tile, q_lds + wid * DHEAD, p_lds + wid * 65, kpool, vpool,
        page_table, slot, kv_len, rg.lo_tok, kvh, KVH, page, max_pages,
        scale, threadIdx.x, lane, c0, c1, 0, m, l, o0, o1);

    // ---- emit ----
    if (split == 1) {
        const float linv = l > 0.f ? 1.f / l : 0.f;
        decode_store(out, S_idx, qh, Hq, lane, fragout, o0 * linv,
                     o1 * linv);
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
    // wave `wid` reduces its head, lane covers dims (2*lane, 2*lane+1)
    const int64_t sh = (int64_t)S_idx * Hq + qh;
    decode_merge_store(out, o_part + sh * split * DHEAD,
                       ml_part + sh * split * 2, split, S_idx, qh, Hq, lane,
                       fragout);
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
    decode_merge_store(out, o_part + (int64_t)sh * split * DHEAD,
                       ml_part + (int64_t)sh * split * 2, split, sh / Hq,
                       sh % Hq, Hq, lane, fragout);
}

extern "C" int decode_attn_bf16(
    void* out, void* o_part, void* ml_part, const void* q,
    const void* kpool, const void* vpool, const void* page_table,
    const void* slot_ids, const void* seq_lens, int S, int Hq, int KVH,
    int page, int max_pages, float scale, int64_t q_stride, int split,
    int window, int chunk, void* sem, int fragout, hipStream_t stream)
{
    const int G = Hq / KVH;
    const int lds = decode_tile_bytes(chunk) + G * DHEAD * 4 + G * 65 * 4;
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
