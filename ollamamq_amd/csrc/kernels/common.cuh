// Shared device helpers and the layout contracts every kernel file here
// depends on: the activation-fragment ("frag") layout, the FP8 weight pack
// and the paged KV pool addressing.  This header is the ONLY definition of
// each; the
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
// FP8 weight pack (OCP e4m3fn codes, one byte per element): the same
// 32-row tiles and 64-wide k-blocks as the bf16 pack, but a k-block is two
// 16-byte units per lane instead of four, and each unit carries TWO of the
// lane's 8-element MFMA fragments: W[t*32 + r][k], k = b*64 + j*16 + h*8 + e,
// sits in 16-byte unit ((t*NB + b)*2 + (j >> 1))*64 + h*32 + r at byte
// (j & 1)*8 + e.  One dwordx4 load therefore feeds fragments j = 2*jj and
// 2*jj + 1 of the lane (ops/hip.py pack_weight_fp8 spells the same order).
// The per-row dequantisation scales are a separate fp32 vector in PACK row
// order: scale[t*32 + r] belongs to the row stored as row r of tile t.
// ---------------------------------------------------------------------------
// byte offset of W[t*32 + r][k] in a packed fp8 tile stream, NB = K/64
DEV int64_t fp8_pack_off(int t, int r, int k, int NB) {
    const int b = k >> 6, j = (k >> 4) & 3, h = (k >> 3) & 1, e = k & 7;
    return ((((int64_t)t * NB + b) * 2 + (j >> 1)) * 64 + h * 32 + r) * 16
           + (j & 1) * 8 + e;
}

// 8 e4m3fn codes (two dwords, ascending k) -> 8 bf16.  v_cvt_pk_f32_fp8
// widens two codes exactly; every e4m3 value fits bf16's 8 significant
// bits, so keeping the high half of each fp32 is exact as well (no
// rounding happens anywhere: subnormal codes are normal fp32 numbers).
DEV bf16x8 fp8x8_to_bf16x8(unsigned lo, unsigned hi) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;
    union { u32x4_t u; bf16x8 v; } out;
    const f32x2 f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false);
    const f32x2 f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const f32x2 f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false);
    const f32x2 f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    // v_perm_b32 selector 0x07060302: {hi16(first arg), hi16(second arg)}
    out.u.x = __builtin_amdgcn_perm(__float_as_uint(f0.y),
                                    __float_as_uint(f0.x), 0x07060302u);
    out.u.y = __builtin_amdgcn_perm(__float_as_uint(f1.y),
                                    __float_as_uint(f1.x), 0x07060302u);
    out.u.z = __builtin_amdgcn_perm(__float_as_uint(f2.y),
                                    __float_as_uint(f2.x), 0x07060302u);
    out.u.w = __builtin_amdgcn_perm(__float_as_uint(f3.y),
                                    __float_as_uint(f3.x), 0x07060302u);
    return out.v;
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
