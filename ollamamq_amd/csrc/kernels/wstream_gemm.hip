// gfx950 weight-streaming decode GEMM: y[M,N] = x[M,K] @ W[N,K]^T, M <= 64.
//
// The decode projections are pure weight streaming (each weight byte is
// used M<=64 times; compute is nothing next to the 8 TB/s HBM pull), and
// round-1 measured hipBLASLt at 1.8-4.6 TB/s on these shapes with a
// ~19 us floor on qkv/o (profiles/r01_decode_step_budget.md).  Two
// hand-written attempts also lost:
//  * fragment-direct (removed; measured history in NOTES.md): MFMA-layout
//    loads are 16 B/lane at 8 KB row stride -> cold misses over-fetched
//    ~4x;
//  * LDS-staged: full-line loads, but __syncthreads() carries a vmcnt(0)
//    (cdna_hip_programming.md "Pipelining across barriers"), draining the
//    prefetch ring every chunk -> 87% SQ_WAIT_ANY.
//
// This kernel removes the conflict at the source: the weights are OURS,
// so they are stored pre-packed in MFMA fragment order (ops/hip.py
// pack_weight): each 32-row tile t of W is one frag-layout image
// (common.cuh), tiles back to back.
// The stream is then PERFECTLY linear: each wave reads consecutive 1 KiB
// vectors (full 128 B line use per instruction), tagged non-temporal
// (MI355X_MICROARCH "nt-weights": one-time-read stream, -18% landed
// traffic), with no LDS staging, no barriers, and a register prefetch one
// 4 KiB iteration deep per wave (8 waves x ~2 blocks/CU ~= 64 KiB in
// flight/CU -> "streaming" regime, MICROARCH price-table preamble).
//
// Geometry: grid (N/32, ksplit) x 512 threads (8 waves).  The K/64
// k-blocks are range-partitioned over ksplit*8 waves (uneven ranges OK:
// any K%64==0, N%32==0, M<=64).  Wave partials meet in a single
// end-of-kernel LDS reduce (the ONE barrier, after all streaming).
// ksplit>1 writes fp32 partials; k_wstream_combine folds them (+bias).
//
// Weights may also be FP8 (e4m3) codes with per-row power-of-two scales
// (WF = 1, see k_wstream_gemm): half the stream, widened to bf16 in
// registers in front of the same MFMA sequence.
//
// Activations may arrive and leave in the frag layout (XLDS=2 / yfrag):
// the same fragment order applied to a [32, K] activation, defined with
// frag_off in common.cuh.
#include "common.cuh"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

union u4bf8 { u32x4 u; bf16x8 v; };

// Pure-stream diagnostic: same grid/geometry/addressing as the GEMM but
// only the nt weight loads (no x, no MFMA) — measures this geometry's
// load-path ceiling so kernel iterations know what they are chasing.
// WF: weight format, 0 = bf16 pack (4 units per lane and k-block),
// 1 = fp8 pack (2 units, common.cuh "FP8 weight pack").
template <int WF>
__global__ __launch_bounds__(512) void k_wstream_pure(
    float* __restrict__ sink, const u32x4* __restrict__ wp,
    int N, int K, int ksplit)
{
    const int t = blockIdx.x;
    const int ks = blockIdx.y;
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int NB = K >> 6;
    const int GW = ksplit * 8;
    const int gw = ks * 8 + wid;
    const int b_lo = (int)(((int64_t)gw * NB) / GW);
    const int b_hi = (int)(((int64_t)(gw + 1) * NB) / GW);
    unsigned acc = 0;
    constexpr int UPB = WF ? 2 : 4;        // 16-byte units per lane, block
    const u32x4* wq = wp + (((int64_t)t * NB + b_lo) * UPB) * 64 + lane;
    for (int b = b_lo; b < b_hi; ++b, wq += UPB * 64) {
        u32x4 v0 = __builtin_nontemporal_load(wq);
        u32x4 v1 = __builtin_nontemporal_load(wq + 64);
        acc ^= v0.x ^ v0.w ^ v1.x ^ v1.w;
        if (!WF) {
            u32x4 v2 = __builtin_nontemporal_load(wq + 128);
            u32x4 v3 = __builtin_nontemporal_load(wq + 192);
            acc ^= v2.x ^ v2.w ^ v3.x ^ v3.w;
        }
    }
    if (acc == 0xDEADBEEFu) sink[0] = 1.f;   // never: keeps loads alive
}

extern "C" int wstream_pure_bf16(void* sink, const void* wp, int N, int K,
                                 int ksplit, int wfmt, hipStream_t stream)
{
    dim3 grid(N / 32, ksplit);
    if (wfmt)
        k_wstream_pure<1><<<grid, 512, 0, stream>>>(
            (float*)sink, (const u32x4*)wp, N, K, ksplit);
    else
        k_wstream_pure<0><<<grid, 512, 0, stream>>>(
            (float*)sink, (const u32x4*)wp, N, K, ksplit);
    return (int)hipGetLastError();
}

// MT: m-tiles of 32 rows (1: M<=32, 2: M<=64).
// DEPTH: weight prefetch depth in 4 KiB iterations (1 or 2); 2 doubles
// the b-register ring so a whole iteration's loads stay in flight across
// one full compute iteration (covers ~2x the HBM latency per wave).
// XLDS (requires MT==1): stage the x fragments through a wave-PRIVATE
// LDS tile instead of loading them in MFMA layout.  The direct x
// fragment load is 32 rows x 16 B at an 8 KB stride = 32 cache-line
// requests per instruction x 4 per iteration; staged, the global x read
// is 4 coalesced instructions (8 lines each), a dense ds_write and a
// minimum-phase swizzled ds_read (u = r*8 + (c ^ (r&7))).  Wave-private
// double-buffered tiles -> NO barrier anywhere in the stream (a
// __syncthreads would drain vmcnt and kill the weight prefetch).
// GU (requires MT==1, ksplit==1): fused gate_up@SwiGLU.  The weights are
// packed with gate and up INTERLEAVED (tile t = 16 gate rows f=t*16..+16
// then the 16 matching up rows — ops/hip.py pack_weight_gu), so each
// block's 32-column output tile holds the (gate, up) pairs of 16 ffn
// columns; the epilogue computes silu(g)*u and stores [M, 16] of the
// activation directly.  Kills the separate swiglu kernel (9.7 us x 32
// layers/step in the r02 trace) and the gate_up intermediate round-trip.
// Fused-rmsnorm chain extensions (all nullable; tp=1 decode path):
//  * rstd_parts/rstd_nt: per-tile sum-of-squares partials of the RAW
//    residual state x (written by the producing GEMM's epilogue).  The
//    epilogue scales row m by rstd[m] = rsqrt(sum*inv_h + eps) — the
//    norm WEIGHT is folded into the packed W at pack time, so
//    y = rmsnorm(x)@W' without any rmsnorm kernel in the step.
//  * res_in/sq_parts: epilogue adds the residual stream (in-place safe:
//    each (m,n) is read+written by exactly one block) and emits this
//    block's sum-of-squares partials for the NEXT GEMM's rstd.
// RoPE/KV-append epilogue bundle (RP=1 qkv GEMM): the packed qkv
// weight is PAIR-ORDERED per head (16 lo-dims then their 16 hi-dims,
// ops/hip.py pack_weight_qkv_rope), so each 32-col output tile holds
// complete rotation pairs; the epilogue rotates q/k with the host
// cos/sin tables and writes k/v straight into the paged KV pool —
// the separate rope_append kernel (8.6 us x layers/step in the r02
// trace) disappears from the decode step.
struct RopeEpi {
    const float* cos_t;   // [max_ctx, 64]
    const float* sin_t;
    const int* pos;       // [M] position of this step's token
    const int* slot;      // [M] kv slot per row
    const int* ptab;      // page table [slots, maxp]
    bf16* kp;             // this layer's K pool base
    bf16* vp;
    int nl, nkl, psz, maxp;
};

// Spill one wave's 32x32 fp32 accumulator tile (MFMA C layout: col =
// lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)) to its red8 slab for the
// cross-wave reduce.  The leading barrier closes whatever read smem last
// (the streaming epoch's x tiles, or the previous m-tile's reduce); the
// trailing one publishes all 8 slabs.
DEV void spill_acc(float (*red8)[32][32], const f32x16& acc, int wid,
                   int lane) {
    __syncthreads();
    #pragma unroll
    for (int r = 0; r < 16; r++) {
        const int crow = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        red8[wid][crow][lane & 31] = acc[r];
    }
    __syncthreads();
}

// WF (weight format): 0 = bf16 pack; 1 = fp8 pack (OCP e4m3fn codes,
// common.cuh "FP8 weight pack") with a per-row fp32 power-of-two scale
// vector `wscale` in PACK row order.  The fp8 variant differs only in how
// B fragments reach registers: a k-block is two 16-byte loads per lane,
// each widened in registers to two bf16 fragments that feed the SAME
// bf16 MFMA sequence over the same wave k-ranges in the same ascending
// order.  The scale multiplies the cross-wave-reduced sum before anything
// else in the epilogue; a power of two commutes with every fp32 rounding,
// so the result is bit-equal to the bf16 kernel over the dequantised
// weights.  A k-block being half the bytes, the fp8 stream keeps TWO
// k-blocks in flight per wave (the two-slot ring of DEPTH == 2: the same
// 4 KiB and the same 4 load registers as the bf16 DEPTH == 1 stream);
// fp8 is instantiated for DEPTH == 1 only.
template <int MT, int DEPTH = 1, int XLDS = 0, int GU = 0, int RP = 0,
          int WF = 0>
__global__ __launch_bounds__(512) void k_wstream_gemm(
    bf16* __restrict__ y,            // [M, N] (ksplit == 1)
    float* __restrict__ part,        // [ksplit, M, N] (ksplit > 1)
    const bf16* __restrict__ x,      // [M, K], row stride xs
    const u32x4* __restrict__ wp,    // packed W (see header)
    const bf16* __restrict__ bias,   // [N] or null (ksplit==1 path)
    int M, int N, int K, int64_t xs, int ksplit,
    const float* __restrict__ rstd_parts, int rstd_nt, float inv_h,
    float eps, const bf16* __restrict__ res_in,
    float* __restrict__ sq_parts, RopeEpi rp = {}, int yfrag = 0,
    const float* __restrict__ wscale = nullptr)   // [N], WF == 1 only
{
    static_assert(!WF || DEPTH == 1, "fp8 packs: DEPTH == 1 only");
    constexpr int UPB = WF ? 2 : 4;        // 16-byte units per lane, block
    constexpr int RING = (DEPTH == 2 || WF) ? 2 : 1;   // k-blocks in flight
    const int t = blockIdx.x;              // n-tile (32 cols of y)
    const int ks = blockIdx.y;
    const int tid = threadIdx.x;
    const int wid = tid >> 6;
    const int lane = tid & 63;
    const int row = lane & 31;
    const int khalf = (lane >> 5) * 8;

    const int NB = K >> 6;                 // 64-elem k-blocks
    const int GW = ksplit * 8;             // waves across k
    const int gw = ks * 8 + wid;
    const int b_lo = (int)(((int64_t)gw * NB) / GW);
    const int b_hi = (int)(((int64_t)(gw + 1) * NB) / GW);

    // clamp so every lane loads valid x rows (rows >= M never stored;
    // per-lane conditional loads would branch+vmcnt(0) per chunk)
    const int ar0 = row < M ? row : (M > 0 ? M - 1 : 0);
    const bf16* xr0 = x + (int64_t)ar0 * xs + khalf;
    const bf16* xr1 = nullptr;
    if (MT == 2) {
        const int r1 = 32 + row;
        const int ar1 = r1 < M ? r1 : (M - 1);
        xr1 = x + (int64_t)ar1 * xs + khalf;
    }

    // dynamic LDS: 32 KiB (wave-partial reduce) or 64 KiB (XLDS adds 8
    // double-buffered 4 KiB wave-private x tiles, reduce space aliased —
    // a __syncthreads separates the stream epoch from the reduce epoch)
    extern __shared__ __align__(16) char smem[];

    f32x16 acc0 = {}, acc1 = {};
    if (b_lo < b_hi) {
        const u32x4* wbase = wp + ((int64_t)t * NB * UPB) * 64 + lane;
        u4bf8 br[RING][UPB];
        bf16x8 a0[2], a1[2], a2[2], a3[2];
        const u4bf8* xf = reinterpret_cast<const u4bf8*>(x);
        auto lda16 = [&](bf16x8* d, int b, int off) {
            if (XLDS == 2) {   // frag input: linear like the weights
                const int64_t u = ((int64_t)b * 4 + (off >> 4)) * 64
                                  + lane;
                d[0] = xf[u].v;
                if (MT == 2)   // second 32-row frag half
                    d[1] = xf[u + (int64_t)4 * K].v;
                return;
            }
            const int64_t k = ((int64_t)b << 6) + off;
            d[0] = *reinterpret_cast<const bf16x8*>(xr0 + k);
            if (MT == 2) d[1] = *reinterpret_cast<const bf16x8*>(xr1 + k);
        };
        auto lda = [&](int b) {
            lda16(a0, b, 0);
            lda16(a1, b, 16);
            lda16(a2, b, 32);
            lda16(a3, b, 48);
        };
        // clamped prefetch: an over-the-end refill re-reads a valid block
        // instead of branching per lane (the tail never computes it)
        auto ldb = [&](int s, int b) {
            const u32x4* q = wbase + (int64_t)(b < b_hi ? b : b_hi - 1)
                                     * (UPB * 64);
            br[s][0].u = __builtin_nontemporal_load(q);
            br[s][1].u = __builtin_nontemporal_load(q + 64);
            if constexpr (!WF) {
                br[s][2].u = __builtin_nontemporal_load(q + 128);
                br[s][3].u = __builtin_nontemporal_load(q + 192);
            }
        };
        auto compute = [&](int s) {
            bf16x8 vb0, vb1, vb2, vb3;
            if constexpr (WF) {      // unit jj holds fragments 2*jj (.xy), 2*jj+1 (.zw)
                vb0 = fp8x8_to_bf16x8(br[s][0].u.x, br[s][0].u.y);
                vb1 = fp8x8_to_bf16x8(br[s][0].u.z, br[s][0].u.w);
                vb2 = fp8x8_to_bf16x8(br[s][1].u.x, br[s][1].u.y);
                vb3 = fp8x8_to_bf16x8(br[s][1].u.z, br[s][1].u.w);
            } else {
                vb0 = br[s][0].v, vb1 = br[s][1].v;
                vb2 = br[s][2].v, vb3 = br[s][3].v;
            }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a0[0], vb0, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a1[0], vb1, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a2[0], vb2, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                a3[0], vb3, acc0, 0, 0, 0);
            if (MT == 2) {
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    a0[1], vb0, acc1, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    a1[1], vb1, acc1, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    a2[1], vb2, acc1, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                    a3[1], vb3, acc1, 0, 0, 0);
            }
        };
        if (XLDS == 1) {
            // --- LDS-staged x fragments (MT==1 only) ---
            bf16x8 xs4[4];
            auto glbx = [&](int b) {       // 4 coalesced reads: 8 rows
                const int64_t kk = (int64_t)b << 6;   // x 128 B each
                #pragma unroll
                for (int i2 = 0; i2 < 4; i2++) {
                    const int r = 8 * i2 + (lane >> 3);
                    const int ar = r < M ? r : (M - 1);
                    xs4[i2] = *reinterpret_cast<const bf16x8*>(
                        x + (int64_t)ar * xs + kk + (lane & 7) * 8);
                }
            };
            auto dswx = [&](int s) {       // dense swizzled tile write
                bf16* tile = reinterpret_cast<bf16*>(smem)
                             + (wid * 2 + s) * 2048;
                #pragma unroll
                for (int i2 = 0; i2 < 4; i2++) {
                    const int u = (8 * i2 + (lane >> 3)) * 8
                                  + ((lane & 7) ^ (lane >> 3));
                    *reinterpret_cast<bf16x8*>(tile + u * 8) = xs4[i2];
                }
            };
            auto dsrx = [&](int s) {       // min-phase fragment reads
                const bf16* tile = reinterpret_cast<const bf16*>(smem)
                                   + (wid * 2 + s) * 2048;
                const int r = lane & 31;
                #pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int c = j * 2 + (lane >> 5);
                    const int u = r * 8 + (c ^ (r & 7));
                    bf16x8 v = *reinterpret_cast<const bf16x8*>(
                        tile + u * 8);
                    if (j == 0) a0[0] = v;
                    else if (j == 1) a1[0] = v;
                    else if (j == 2) a2[0] = v;
                    else a3[0] = v;
                }
            };
            ldb(0, b_lo);
            if constexpr (RING == 2) ldb(1, b_lo + 1);
            glbx(b_lo);
            dswx(0);
            int b = b_lo;
            if constexpr (RING == 1) {
                for (; b < b_hi - 1; ++b) {
                    const int s = (b - b_lo) & 1;
                    dsrx(s);
                    compute(0);
                    ldb(0, b + 1);
                    glbx(b + 1);
                    dswx(s ^ 1);
                }
                dsrx((b - b_lo) & 1);
                compute(0);
            } else {
                // two weight slots: block b_lo + i uses weight slot and x
                // tile i & 1, in the same ascending order as above
                for (; b + 2 < b_hi; b += 2) {
                    dsrx(0);
                    compute(0);
                    ldb(0, b + 2);
                    glbx(b + 1);
                    dswx(1);
                    dsrx(1);
                    compute(1);
                    ldb(1, b + 3);
                    glbx(b + 2);
                    dswx(0);
                }
                dsrx(0);
                compute(0);
                if (b + 1 < b_hi) {
                    glbx(b + 1);
                    dswx(1);
                    dsrx(1);
                    compute(1);
                }
            }
        } else {
            ldb(0, b_lo);
            if constexpr (RING == 2) ldb(1, b_lo + 1);
            lda(b_lo);
            int b = b_lo;
            if constexpr (RING == 1) {
                for (; b < b_hi - 1; ++b) {
                    compute(0);
                    ldb(0, b + 1);
                    lda(b + 1);
                }
                compute(0);
            } else {
                for (; b + 2 < b_hi; b += 2) {
                    compute(0);
                    ldb(0, b + 2);
                    lda(b + 1);
                    compute(1);
                    ldb(1, b + 3);
                    lda(b + 2);
                }
                compute(0);
                if (b + 1 < b_hi) {
                    lda(b + 1);
                    compute(1);
                }
            }
        }
    }

    // ---- reduce 8 wave partials through LDS (aliases the x tiles: the
    // barrier closes the streaming epoch before anyone writes) ----
    float (*red8)[32][32] = reinterpret_cast<float (*)[32][32]>(smem);
    // rmsnorm scale of the raw-residual input: sum this row's sq
    // partials from the producing GEMM (L2-hot, overlapped with other
    // waves' stream drain), publish rstd through the smem tail
    float* rstd_sh = reinterpret_cast<float*>(
        smem + (XLDS == 1 ? 16 * 4096 : 8 * 32 * 32 * 4));
    if (rstd_parts) {
        // parallel partial fold: 8-16 lanes per row (each <= nt/L loads,
        // independent), group-reduced with wave shuffles — a serial
        // 32-thread loop here measurably stalled short-stream blocks.
        // MT==2 folds 64 rows with 8 lanes each (512 threads exactly).
        const int L = MT == 2 ? 8 : 16;
        const int m2 = tid / L, c2 = tid % L;
        float s = 0.f;
        if (m2 < MT * 32)
            for (int i = c2; i < rstd_nt; i += L)
                s += rstd_parts[(int64_t)m2 * rstd_nt + i];
        #pragma unroll
        for (int off = 8; off; off >>= 1)
            if (off < L) s += __shfl_down(s, off, 64);
        if (m2 < MT * 32 && c2 == 0)
            rstd_sh[m2] = rsqrtf(s * inv_h + eps);
    }
    if (GU) {
        const int F = N >> 1;                  // ffn width
        for (int mt = 0; mt < MT; ++mt) {
            spill_acc(red8, mt ? acc1 : acc0, wid, lane);
            const int m = tid >> 4, c = tid & 15;  // 512 thr = 32 x 16
            const int gm = m + mt * 32;
            if (gm < M) {
                float sg = 0.f, su = 0.f;
                #pragma unroll
                for (int wv = 0; wv < 8; wv++) {
                    sg += red8[wv][m][c];
                    su += red8[wv][m][c + 16];
                }
                if constexpr (WF) {            // pack row order: GU tile
                    sg *= wscale[t * 32 + c];
                    su *= wscale[t * 32 + 16 + c];
                }
                if (rstd_parts) {              // MT==1 chain only
                    const float rs = rstd_sh[gm];  // pre-silu: nonlinear
                    sg *= rs;
                    su *= rs;
                }
                const float act = (sg / (1.f + __expf(-sg))) * su;
                const int fc = t * 16 + c;
                y[yfrag ? (int64_t)mt * 32 * F + frag_off(m, fc)
                        : (int64_t)gm * F + fc] = __float2bfloat16(act);
            }
        }
        return;
    }
    if (RP) {
        const int qt = rp.nl * 4, kt = rp.nkl * 4;   // tiles per section
        for (int mt = 0; mt < MT; ++mt) {
            spill_acc(red8, mt ? acc1 : acc0, wid, lane);
            if (t < qt + kt) {
                // pair-packed q/k tile: cols {d0+c, d0+64+c}, c<16
                const int m = tid >> 4, c = tid & 15;
                const int gm = m + mt * 32;
                if (gm < M) {
                    const int sec_t = t < qt ? t : t - qt;
                    const int head = sec_t >> 2;
                    const int d0 = (sec_t & 3) * 16;
                    float lo = 0.f, hi = 0.f;
                    #pragma unroll
                    for (int wv = 0; wv < 8; wv++) {
                        lo += red8[wv][m][c];
                        hi += red8[wv][m][c + 16];
                    }
                    if constexpr (WF) {   // pair-ordered like the pack
                        lo *= wscale[t * 32 + c];
                        hi *= wscale[t * 32 + 16 + c];
                    }
                    if (rstd_parts) {
                        const float rs = rstd_sh[gm];
                        lo *= rs;
                        hi *= rs;
                    }
                    if (bias) {  // bias is pair-reordered like the pack
                        lo += __bfloat162float(bias[t * 32 + c]);
                        hi += __bfloat162float(bias[t * 32 + 16 + c]);
                    }
                    const int p = rp.pos[gm];
                    const float co = rp.cos_t[p * 64 + d0 + c];
                    const float si = rp.sin_t[p * 64 + d0 + c];
                    const float rlo = lo * co - hi * si;
                    const float rhi = hi * co + lo * si;
                    if (t < qt) {          // q: standard layout in y
                        bf16* qr = y + (int64_t)gm * N + head * 128;
                        qr[d0 + c] = __float2bfloat16(rlo);
                        qr[64 + d0 + c] = __float2bfloat16(rhi);
                    } else {               // k: rotated, straight to pool
                        bf16* dst = rp.kp + paged_kv_row(
                            rp.ptab, rp.slot[gm], rp.maxp, p, rp.psz,
                            rp.nkl, head);
                        dst[d0 + c] = __float2bfloat16(rlo);
                        dst[64 + d0 + c] = __float2bfloat16(rhi);
                    }
                }
            } else {
                // v tile (plain 32-col order): straight to pool, no rope
                const int sec_t = t - qt - kt;
                const int head = sec_t >> 2;
                const int d0 = (sec_t & 3) * 32;
                #pragma unroll
                for (int ee = 0; ee < 2; ee++) {
                    const int e = tid + ee * 512;
                    const int mr = e >> 5, n = e & 31;
                    const int gm = mr + mt * 32;
                    if (gm < M) {
                        float sv = 0.f;
                        #pragma unroll
                        for (int wv = 0; wv < 8; wv++)
                            sv += red8[wv][mr][n];
                        if constexpr (WF) sv *= wscale[t * 32 + n];
                        if (rstd_parts) sv *= rstd_sh[gm];
                        if (bias)
                            sv += __bfloat162float(bias[t * 32 + n]);
                        bf16* dst = rp.vp + paged_kv_row(
                            rp.ptab, rp.slot[gm], rp.maxp, rp.pos[gm],
                            rp.psz, rp.nkl, head);
                        dst[d0 + n] = __float2bfloat16(sv);
                    }
                }
            }
        }
        return;
    }
    const int n0 = t * 32;
    for (int mt = 0; mt < MT; ++mt) {
        spill_acc(red8, mt ? acc1 : acc0, wid, lane);
        float rsq[2] = {0.f, 0.f};
        #pragma unroll
        for (int ee = 0; ee < 2; ee++) {
            const int e = tid + ee * 512;
            const int mr = e >> 5, n = e & 31;
            const int m = mr + mt * 32;
            if (m < M) {
                float s = 0.f;
                #pragma unroll
                for (int wv = 0; wv < 8; wv++)
                    s += red8[wv][mr][n];
                if constexpr (WF) s *= wscale[n0 + n];
                if (ksplit == 1) {
                    if (rstd_parts) s *= rstd_sh[m];
                    if (bias) s += __bfloat162float(bias[n0 + n]);
                    const int64_t yo =
                        yfrag ? (int64_t)mt * 32 * N + frag_off(mr, n0 + n)
                              : (int64_t)m * N + n0 + n;
                    if (res_in) {
                        s += __bfloat162float(res_in[yo]);
                        rsq[ee] = s * s;
                    }
                    y[yo] = __float2bfloat16(s);
                } else {
                    part[((int64_t)ks * M + m) * N + n0 + n] = s;
                }
            }
        }
        // emit this block's sum-of-squares partials for the mt rows
        if (sq_parts && ksplit == 1) {
            __syncthreads();
            float (*sqt)[32] = reinterpret_cast<float (*)[32]>(smem);
            sqt[tid >> 5][tid & 31] = rsq[0];          // rows 0..15
            sqt[(tid >> 5) + 16][tid & 31] = rsq[1];   // rows 16..31
            __syncthreads();
            if (tid < 32) {
                float s = 0.f;
                #pragma unroll
                for (int n2 = 0; n2 < 32; n2++) s += sqt[tid][n2];
                // m-major [M][n_tiles]: the consumer's fold walks tiles
                // CONTIGUOUSLY (a tile-major layout cost 1 float per
                // 128 B line and ~3 us per consumer block)
                sq_parts[(int64_t)(tid + mt * 32) * gridDim.x + t] = s;
            }
            if (MT == 2 && mt == 0) __syncthreads();  // sqt reused
        }
    }
}

// Host-side bundle of k_wstream_gemm's runtime arguments: the extern "C"
// entry points fill it once and only choose template arguments.
struct WsArgs {
    void* y;
    void* part;
    const void* x;
    const void* wp;
    const void* bias;
    int M, N, K;
    int64_t xs;
    int ksplit;
    const void* rstd_parts;
    int rstd_nt;
    float inv_h, eps;
    const void* res_in;
    void* sq_parts;
    RopeEpi rp;
    int yfrag;
    const void* wscale;   // fp8 pack: [N] fp32 row scales; null = bf16 pack
};

// The one launch site.  Dynamic LDS: the 8-wave reduce space (32 KiB), or
// the 8 double-buffered 4 KiB x tiles it aliases when XLDS == 1 (64 KiB),
// plus the 256 B rstd tail.
template <int MT, int DEPTH, int XLDS, int GU, int RP, int WF>
static void ws_launch_wf(const WsArgs& a, hipStream_t stream)
{
    const int lds = (XLDS == 1 ? 16 * 4096 : 8 * 32 * 32 * 4) + 256;
    dim3 grid(a.N / 32, a.ksplit);
    k_wstream_gemm<MT, DEPTH, XLDS, GU, RP, WF><<<grid, 512, lds, stream>>>(
        (bf16*)a.y, (float*)a.part, (const bf16*)a.x, (const u32x4*)a.wp,
        (const bf16*)a.bias, a.M, a.N, a.K, a.xs, a.ksplit,
        (const float*)a.rstd_parts, a.rstd_nt, a.inv_h, a.eps,
        (const bf16*)a.res_in, (float*)a.sq_parts, a.rp, a.yfrag,
        (const float*)a.wscale);
}

// A scale vector selects the fp8 instantiation of the same geometry.  fp8
// exists at DEPTH == 1 only: the entry points answer WS_ERR_FP8_DEPTH
// before they get here, so nothing is launched for that combination.
constexpr int WS_ERR_FP8_DEPTH = -103;

template <int MT, int DEPTH, int XLDS, int GU, int RP>
static void ws_launch(const WsArgs& a, hipStream_t stream)
{
    if (!a.wscale)
        ws_launch_wf<MT, DEPTH, XLDS, GU, RP, 0>(a, stream);
    else if constexpr (DEPTH == 1)
        ws_launch_wf<MT, 1, XLDS, GU, RP, 1>(a, stream);
}

// Fused gate_up @ SwiGLU over GU-interleaved packed weights.
// N = 2F total weight rows; output is the activation [M, F].
// rstd_parts: optional fused-rmsnorm scale of the raw-residual input.
extern "C" int wstream_gu_bf16(
    void* act, const void* x, const void* wp, int M, int N, int K,
    int64_t xs, int xlds, const void* rstd_parts, int rstd_nt,
    float inv_h, float eps, int yfrag, const void* wscale,
    hipStream_t stream)
{
    const WsArgs a{act, nullptr, x, wp, nullptr, M, N, K, xs, 1,
                   rstd_parts, rstd_nt, inv_h, eps, nullptr, nullptr, {},
                   yfrag, wscale};
    if (M > 32) {
        if (xlds == 2)         // frag chain at batches 33..64
            ws_launch<2, 1, 2, 1, 0>(a, stream);
        else if (rstd_parts || yfrag)
            return -102;       // fusion needs the frag path at MT2
        else
            // generic-path fused gate_up+SwiGLU, direct x loads (unused
            // by default: measured below lib at 64 users)
            ws_launch<2, 1, 0, 1, 0>(a, stream);
    } else if (xlds == 2)
        ws_launch<1, 1, 2, 1, 0>(a, stream);
    else if (xlds == 1)
        ws_launch<1, 1, 1, 1, 0>(a, stream);
    else
        ws_launch<1, 1, 0, 1, 0>(a, stream);
    return (int)hipGetLastError();
}


__global__ __launch_bounds__(256) void k_wstream_combine(
    bf16* __restrict__ y, const float* __restrict__ part,
    const bf16* __restrict__ bias, int64_t total, int64_t mn, int N,
    int ksplit)
{
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int k = 0; k < ksplit; k++) s += part[k * mn + i];
        if (bias) s += __bfloat162float(bias[i % N]);
        y[i] = __float2bfloat16(s);
    }
}

// Tile-structured combine for the fused chain (M <= 32): folds the
// k-split partials, adds the residual stream in place and emits per-tile
// sum-of-squares partials for the next GEMM's rstd.
__global__ __launch_bounds__(256) void k_wstream_combine_tiles(
    bf16* __restrict__ y, const float* __restrict__ part,
    const bf16* __restrict__ res_in, float* __restrict__ sq_parts,
    int M, int N, int ksplit, int yfrag)
{
    const int t = blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ float sqt[32][32];
    const int n0 = t * 32;
    const int mts = (M + 31) >> 5;          // 1 or 2 m-halves
    for (int mt = 0; mt < mts; ++mt) {
        if (mt) __syncthreads();
        #pragma unroll
        for (int ee = 0; ee < 4; ee++) {
            const int e = tid + ee * 256;
            const int mr = e >> 5, n = e & 31;
            const int m = mr + mt * 32;
            float rsq = 0.f;
            if (m < M) {
                float s = 0.f;
                for (int k = 0; k < ksplit; k++)
                    s += part[((int64_t)k * M + m) * N + n0 + n];
                const int64_t yo =
                    yfrag ? (int64_t)mt * 32 * N + frag_off(mr, n0 + n)
                          : (int64_t)m * N + n0 + n;
                if (res_in)
                    s += __bfloat162float(res_in[yo]);
                y[yo] = __float2bfloat16(s);
                rsq = s * s;
            }
            sqt[mr][n] = rsq;
        }
        if (sq_parts) {
            __syncthreads();
            if (tid < 32) {
                float s = 0.f;
                #pragma unroll
                for (int n2 = 0; n2 < 32; n2++) s += sqt[tid][n2];
                sq_parts[(int64_t)(tid + mt * 32) * gridDim.x + t] = s;
            }
        }
    }
}

extern "C" int wstream_gemm_bf16(
    void* y, void* part, const void* x, const void* wp, const void* bias,
    int M, int N, int K, int64_t xs, int ksplit, int depth, int xlds,
    const void* rstd_parts, int rstd_nt, float inv_h, float eps,
    const void* res_in, void* sq_parts, int yfrag, const void* wscale,
    hipStream_t stream)
{
    if (ksplit > 1 && rstd_parts) return -100;     // fused rstd needs ks==1
    if (wscale && depth != 1) return WS_ERR_FP8_DEPTH;
    // the residual add and the sq partials belong to whoever writes y:
    // this kernel at ksplit == 1, the tile combine below otherwise
    const WsArgs a{y, part, x, wp, bias, M, N, K, xs, ksplit,
                   rstd_parts, rstd_nt, inv_h, eps,
                   ksplit == 1 ? res_in : nullptr,
                   ksplit == 1 ? sq_parts : nullptr, {}, yfrag, wscale};
    if (M <= 32) {
        if (xlds == 2)
            ws_launch<1, 1, 2, 0, 0>(a, stream);
        else if (xlds == 1)
            ws_launch<1, 1, 1, 0, 0>(a, stream);
        else if (depth == 2)
            ws_launch<1, 2, 0, 0, 0>(a, stream);
        else
            ws_launch<1, 1, 0, 0, 0>(a, stream);
    } else {
        if (xlds == 2)
            ws_launch<2, 1, 2, 0, 0>(a, stream);
        else if (rstd_parts || res_in || sq_parts || yfrag)
            return -101;           // fusion needs the frag path at MT2
        else if (depth == 2)
            ws_launch<2, 2, 0, 0, 0>(a, stream);
        else
            ws_launch<2, 1, 0, 0, 0>(a, stream);
    }
    if (ksplit > 1) {
        if (res_in || sq_parts) {
            k_wstream_combine_tiles<<<N / 32, 256, 0, stream>>>(
                (bf16*)y, (const float*)part, (const bf16*)res_in,
                (float*)sq_parts, M, N, ksplit, yfrag);
        } else {
            const int64_t mn = (int64_t)M * N;
            const int64_t want = (mn + 255) / 256;
            const int blocks = (int)(want < 1024 ? want : 1024);
            k_wstream_combine<<<blocks, 256, 0, stream>>>(
                (bf16*)y, (const float*)part, (const bf16*)bias, mn, mn,
                N, ksplit);
        }
    }
    return (int)hipGetLastError();
}



// qkv GEMM with fused RoPE + paged KV append (fused decode chain):
// q lands rotated in y's standard layout; k/v land in the paged pool.
extern "C" int wstream_qkv_rope_bf16(
    void* y, const void* x, const void* wp, const void* bias,
    int M, int N, int K, int64_t xs,
    const void* rstd_parts, int rstd_nt, float inv_h, float eps,
    const void* rcos, const void* rsin, const void* pos,
    const void* slot, const void* ptab, void* kp, void* vp,
    int nl, int nkl, int psz, int maxp, int xf, const void* wscale,
    hipStream_t stream)
{
    const RopeEpi rp{(const float*)rcos, (const float*)rsin,
                     (const int*)pos, (const int*)slot, (const int*)ptab,
                     (bf16*)kp, (bf16*)vp, nl, nkl, psz, maxp};
    const WsArgs a{y, nullptr, x, wp, bias, M, N, K, xs, 1,
                   rstd_parts, rstd_nt, inv_h, eps, nullptr, nullptr, rp,
                   0, wscale};
    if (xf && M > 32)
        ws_launch<2, 1, 2, 0, 1>(a, stream);
    else if (xf)
        ws_launch<1, 1, 2, 0, 1>(a, stream);
    else
        ws_launch<1, 1, 0, 0, 1>(a, stream);
    return (int)hipGetLastError();
}
