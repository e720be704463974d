// gfx950 decode attention, block-split: all NSEG KV segments of one
// (sequence, kv-head) in ONE block, partials merged through LDS.
//
// decode_attn.hip's split path runs one 4-wave block per segment, writes
// fp32 (o, m, l) partials to global memory and launches k_decode_combine
// to read them back.  At S*KVH >= 128 the NSEG blocks of a (sequence,
// kv-head) already amount to one CU's worth of waves and LDS, so here they
// are one block of NSEG*GT waves: each group of GT waves sweeps one segment
// on tiles of its own (same waves, same tiles, same loads in flight, same
// per-segment arithmetic: decode_attn.cuh decode_attn_segment), and the GT
// waves of segment 0 merge the partials from LDS with decode_merge_store,
// the expressions of k_decode_combine in the same order, so the output is
// bit-identical to the two-kernel path.  No global partials, no fence, no
// ticket, no second launch; q, slot_ids and seq_lens are read once per
// (sequence, kv-head).
//
// This file also instantiates both decode kernels for e4m3 KV pools
// (common.cuh KvFmt<1>): k_decode_attn_blk at every BLK_INSTANCES entry and
// k_decode_attn (decode_attn.cuh) at every (G, chunk), entries *_kv8.
#include "decode_attn.cuh"

// dynamic LDS: q [GT][128] f32, then per segment K tile, V tile, p [GT][65]
constexpr int blk_seg_bytes(int GT, int CH) {
    return (decode_tile_bytes(CH) + GT * 65 * 4 + 15) & ~15;
}
constexpr int blk_lds_bytes(int GT, int CH, int NSEG) {
    return GT * DHEAD * 4 + NSEG * blk_seg_bytes(GT, CH);
}

// grid: (n_seqs, KVH); block: NSEG*GT*64 threads, wave w = segment w / GT,
// head w % GT.  Barriers are block-wide, so every segment runs the longest
// segment's round count and no wave returns before the last barrier.
template <int GT, int CH, int NSEG, int KVF = 0>
__global__ __launch_bounds__(NSEG * GT * 64, 1) void k_decode_attn_blk(
    bf16* __restrict__ out,               // [S, Hq, D] or frag layout
    const bf16* __restrict__ q,           // [S, Hq, D] (row stride qs)
    const typename KvFmt<KVF>::elem* __restrict__ kpool, // [P][KVH][page][D]
    const typename KvFmt<KVF>::elem* __restrict__ vpool,
    const int* __restrict__ page_table,   // [slots][max_pages]
    const int* __restrict__ slot_ids,     // [S]
    const int* __restrict__ seq_lens,     // [S] (kv length incl. this tok)
    int Hq, int KVH, int page, int max_pages, float scale,
    int64_t qs, int window, int fragout)
{
    const int S_idx = blockIdx.x;
    const int kvh = blockIdx.y;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int seg = wid / GT;
    const int hw = wid % GT;              // head wave within the segment
    const int qh = kvh * GT + hw;

    const int slot = slot_ids[S_idx];
    const int kv_len = seq_lens[S_idx];
    const DecodeRange rg = decode_range(kv_len, window, CH);
    const int c0 = decode_seg_bound(rg, seg, NSEG);
    const int c1 = decode_seg_bound(rg, seg + 1, NSEG);
    // floor-interpolated bounds: the longest segment has ceil(n_act / NSEG)
    // chunks.  Block-uniform by construction (no per-wave term).
    const int n_rounds = rg.n_act > 0 ? (rg.n_act + NSEG - 1) / NSEG : 0;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* q_lds = reinterpret_cast<float*>(smem);               // [GT][128]
    char* seg0 = smem + GT * DHEAD * 4;
    bf16* k_tile = reinterpret_cast<bf16*>(seg0 + seg * blk_seg_bytes(GT, CH));
    bf16* v_tile = k_tile + CH * DKROW;
    // p row is per-LANE (65 = 64+pad), see k_decode_attn
    float* p_lds = reinterpret_cast<float*>(v_tile + CH * DKROW); // [GT][65]

    // stage q once per block (fp32 in LDS: repeated broadcast reads)
    if (seg == 0) {
        const bf16* qsrc = q + (int64_t)S_idx * qs + (int64_t)qh * DHEAD;
        q_lds[hw * DHEAD + lane] = bf2f(qsrc[lane]);
        q_lds[hw * DHEAD + lane + 64] = bf2f(qsrc[lane + 64]);
    }
    __syncthreads();

    float m = -3.0e38f, l = 0.f, o0 = 0.f, o1 = 0.f;
    decode_attn_segment<GT, CH, true, KVF>(
        k_tile, v_tile, q_lds + hw * DHEAD, p_lds + hw * 65, kpool, vpool,
        page_table, slot, kv_len, rg.lo_tok, kvh, KVH, page, max_pages,
        scale, (int)threadIdx.x - seg * GT * 64, lane, c0, c1, n_rounds,
        m, l, o0, o1);

    // ---- merge through LDS: the tiles are dead, reuse segment 0's.
    // o [GT][NSEG][128] then (m, l) [GT][NSEG][2]: NSEG*GT*520 B <= 8320 B,
    // inside one K tile (8448 B at CH 32).
    static_assert(NSEG * GT * (DHEAD + 2) * 4 <= CH * DKROW * 2,
                  "merge scratch must fit the K tile it reuses");
    __syncthreads();              // every wave done with every tile
    float* o_mrg = reinterpret_cast<float*>(seg0);
    float* ml_mrg = o_mrg + GT * NSEG * DHEAD;
    {
        const int pi = hw * NSEG + seg;
        o_mrg[pi * DHEAD + 2 * lane] = o0;
        o_mrg[pi * DHEAD + 2 * lane + 1] = o1;
        ml_mrg[pi * 2] = m;
        ml_mrg[pi * 2 + 1] = l;
    }
    __syncthreads();
    if (seg == 0)
        decode_merge_store(out, o_mrg + hw * NSEG * DHEAD,
                           ml_mrg + hw * NSEG * 2, NSEG, S_idx, qh, Hq, lane,
                           fragout);
}

// Instantiated: NSEG in {2, 4} with NSEG * GT <= 16 waves, at the chunk
// ops/hip.py _decode_chunk picks (32 for G = 1, 64 otherwise).  X(GT, CH,
// NSEG) is expanded by both entry points below.
#define BLK_INSTANCES(X)                                                  \
    X(1, 32, 2) X(2, 64, 2) X(3, 64, 2) X(4, 64, 2)                       \
    X(5, 64, 2) X(6, 64, 2) X(7, 64, 2) X(8, 64, 2)                       \
    X(1, 32, 4) X(2, 64, 4) X(3, 64, 4) X(4, 64, 4)

// Opt in to dynamic LDS above 64 KB for one instantiation; call once per
// (G, chunk, split) before its first launch.  Returns the runtime's error
// when it refuses the size (the caller then keeps the two-kernel path), or
// hipErrorInvalidValue for a combination that is not instantiated.
template <int KVF>
static int blk_prepare(int G, int chunk, int split)
{
#define BLK_PREPARE(GT, CH, NSEG)                                         \
    if (G == GT && chunk == CH && split == NSEG)                          \
        return (int)hipFuncSetAttribute(                                  \
            (const void*)k_decode_attn_blk<GT, CH, NSEG, KVF>,            \
            hipFuncAttributeMaxDynamicSharedMemorySize,                   \
            blk_lds_bytes(GT, CH, NSEG));
    BLK_INSTANCES(BLK_PREPARE)
#undef BLK_PREPARE
    return (int)hipErrorInvalidValue;
}

template <int KVF>
static int blk_launch(
    void* out, const void* q, const void* kpool, const void* vpool,
    const void* page_table, const void* slot_ids, const void* seq_lens,
    int S, int Hq, int KVH, int page, int max_pages, float scale,
    int64_t q_stride, int split, int window, int chunk, int fragout,
    hipStream_t stream)
{
    typedef const typename KvFmt<KVF>::elem* pool_t;
    const int G = Hq / KVH;
    dim3 grid(S, KVH);
#define BLK_LAUNCH(GT, CH, NSEG)                                          \
    if (G == GT && chunk == CH && split == NSEG) {                        \
        k_decode_attn_blk<GT, CH, NSEG, KVF>                              \
            <<<grid, NSEG * GT * 64, blk_lds_bytes(GT, CH, NSEG), stream>>>( \
            (bf16*)out, (const bf16*)q, (pool_t)kpool, (pool_t)vpool,     \
            (const int*)page_table,                                       \
            (const int*)slot_ids, (const int*)seq_lens, Hq, KVH, page,    \
            max_pages, scale, q_stride, window, fragout);                 \
        return (int)hipGetLastError();                                    \
    }
    BLK_INSTANCES(BLK_LAUNCH)
#undef BLK_LAUNCH
    return (int)hipErrorInvalidValue;
}

extern "C" int decode_attn_blk_prepare(int G, int chunk, int split)
{
    return blk_prepare<0>(G, chunk, split);
}

extern "C" int decode_attn_blk_bf16(
    void* out, const void* q, const void* kpool, const void* vpool,
    const void* page_table, const void* slot_ids, const void* seq_lens,
    int S, int Hq, int KVH, int page, int max_pages, float scale,
    int64_t q_stride, int split, int window, int chunk, int fragout,
    hipStream_t stream)
{
    return blk_launch<0>(out, q, kpool, vpool, page_table, slot_ids,
                         seq_lens, S, Hq, KVH, page, max_pages, scale,
                         q_stride, split, window, chunk, fragout, stream);
}

// ---- e4m3 KV pools ----
extern "C" int decode_attn_blk_prepare_kv8(int G, int chunk, int split)
{
    return blk_prepare<1>(G, chunk, split);
}

extern "C" int decode_attn_blk_kv8(
    void* out, const void* q, const void* kpool, const void* vpool,
    const void* page_table, const void* slot_ids, const void* seq_lens,
    int S, int Hq, int KVH, int page, int max_pages, float scale,
    int64_t q_stride, int split, int window, int chunk, int fragout,
    hipStream_t stream)
{
    return blk_launch<1>(out, q, kpool, vpool, page_table, slot_ids,
                         seq_lens, S, Hq, KVH, page, max_pages, scale,
                         q_stride, split, window, chunk, fragout, stream);
}

// one block per segment + k_decode_combine; sem must be null (the in-launch
// combine is not instantiated for e4m3 pools)
extern "C" int decode_attn_kv8(
    void* out, void* o_part, void* ml_part, const void* q,
    const void* kpool, const void* vpool, const void* page_table,
    const void* slot_ids, const void* seq_lens, int S, int Hq, int KVH,
    int page, int max_pages, float scale, int64_t q_stride, int split,
    int window, int chunk, void* sem, int fragout, hipStream_t stream)
{
    return decode_attn_launch<1>(
        out, o_part, ml_part, q, kpool, vpool, page_table, slot_ids,
        seq_lens, S, Hq, KVH, page, max_pages, scale, q_stride, split,
        window, chunk, sem, fragout, stream);
}
