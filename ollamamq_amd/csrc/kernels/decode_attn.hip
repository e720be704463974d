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
// The segment sweep, the partial merge, the output store and k_decode_attn
// itself are defined once in decode_attn.cuh; decode_attn_blk.hip is the
// second caller and holds the e4m3-pool instantiations of both kernels.
#include "decode_attn.cuh"

extern "C" int decode_attn_bf16(
    void* out, void* o_part, void* ml_part, const void* q,
    const void* kpool, const void* vpool, const void* page_table,
    const void* slot_ids, const void* seq_lens, int S, int Hq, int KVH,
    int page, int max_pages, float scale, int64_t q_stride, int split,
    int window, int chunk, void* sem, int fragout, hipStream_t stream)
{
    return decode_attn_launch<0>(
        out, o_part, ml_part, q, kpool, vpool, page_table, slot_ids,
        seq_lens, S, Hq, KVH, page, max_pages, scale, q_stride, split,
        window, chunk, sem, fragout, stream);
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
