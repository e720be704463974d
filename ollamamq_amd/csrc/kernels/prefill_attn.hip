// gfx950 MFMA prefill attention over a bf16 paged KV pool: the kernel and
// its launcher are prefill_attn.cuh; this file is the bf16-pool entry.
#include "prefill_attn.cuh"

extern "C" int prefill_attn_bf16(
    void* out, const void* q, const void* kpool, const void* vpool,
    const void* page_table, const void* tile_slot, const void* tile_q0,
    const void* tile_pos0, const void* tile_rows, int n_tiles,
    int Hq, int KVH, int page, int max_pages, float scale, int64_t q_stride,
    int window, hipStream_t stream)
{
    return prefill_attn_launch<0>(
        out, q, kpool, vpool, page_table, tile_slot, tile_q0, tile_pos0,
        tile_rows, n_tiles, Hq, KVH, page, max_pages, scale, q_stride,
        window, stream);
}
