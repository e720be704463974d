// Shared device helpers and the two layout contracts every kernel file
// here depends on: the activation-fragment ("frag") layout and the paged
// KV pool addressing.  This header is the ONLY definition of either; the
// .hip files include it and point here instead of restating the maths.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

typedef __hip_bfloat16 bf16;
typedef __hip_bfloat162 bf162;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define DEV static __device__ __forceinline__

DEV float bf2f(bf16 x) { return __bfloat162float(x); }
DEV bf16 f2bf(float x) { return __float2bfloat16(x); }

// load 8 bf16 (16 B, global or LDS) and widen to 8 floats
DEV void load8f(const bf16* p, float* out) {
    const bf162* v = reinterpret_cast<const bf162*>(p);
    bf162 a = v[0], b = v[1], c = v[2], d = v[3];
    float2 fa = __bfloat1622float2(a), fb = __bfloat1622float2(b);
    float2 fc = __bfloat1622float2(c), fd = __bfloat1622float2(d);
    out[0] = fa.x; out[1] = fa.y; out[2] = fb.x; out[3] = fb.y;
    out[4] = fc.x; out[5] = fc.y; out[6] = fd.x; out[7] = fd.y;
}

// wave64 all-reduce: every lane returns the wave's sum / max
DEV float wave_reduce_sum(float x) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        x += __shfl_down(x, off, 64);
    return __shfl(x, 0, 64);
}

DEV float wave_reduce_max(float x) {
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        x = fmaxf(x, __shfl_down(x, off, 64));
    return __shfl(x, 0, 64);
}

// ---------------------------------------------------------------------------
// Activation-fragment layout ("frag"): the SAME MFMA fragment order the
// weight packs use (ops/hip.py pack_weight), applied to a [32, K]
// activation: element (m, k) with k = b*64 + j*16 + h*8 + e lives at
// 16-byte unit ((b*4 + j)*64 + h*32 + m), elem e.  Producers (GEMM
// epilogues, decode-attention combine, the embedding fragify kernel)
// write it; consumers stream it LINEARLY exactly like packed weights — the
// per-iteration x machinery (32-line scattered loads or LDS staging,
// measured 15-30% on top of the pure stream) disappears.  Buffers are
// always 32 rows; rows >= M hold garbage that MFMA carries in dead
// accumulator rows (never stored).  Batches of 33..64 rows use two such
// buffers back to back: rows 32..63 start at element 32*K.
// A packed [N, K] weight is the same thing per 32-row tile: W[t*32 + r][k]
// sits at unit t*(K/64)*256 + frag_unit(r, k/8), i.e. uint4 index
// ((t*NB + b)*4 + j)*64 + (h*32 + r) with NB = K/64.
// ---------------------------------------------------------------------------
// 16-byte unit of row m's chunk c, where chunk c covers k = c*8 .. c*8+7
DEV int64_t frag_unit(int m, int c) {
    const int b = c >> 3, j = (c >> 1) & 3, h = c & 1;
    return (((int64_t)b * 4 + j) * 64) + h * 32 + m;
}

// element offset of (m, kcol)
DEV int64_t frag_off(int m, int kcol) {
    return frag_unit(m, kcol >> 3) * 8 + (kcol & 7);
}

// ---------------------------------------------------------------------------
// Paged KV pool: one layer's K (or V) pool is [P][KVH][page][128] bf16 and
// page_table is [slots][max_pages].  Returns the element offset of the
// 128-wide row that holds token `pos` of sequence slot `slot` for kv-head
// `head`.  The slot * max_pages product is 64-bit: a table of many slots
// with long contexts passes 2^31 entries before the pool itself does.
// ---------------------------------------------------------------------------
DEV int64_t paged_kv_row(const int* page_table, int slot, int max_pages,
                         int pos, int page, int KVH, int head) {
    const int pg = page_table[(int64_t)slot * max_pages + pos / page];
    return (((int64_t)pg * KVH + head) * page + pos % page) * 128;
}
