// W8A16 MFMA GEMM over an FP8 weight pack, for any M >= 1:
//   y[M, N] = x[M, K] @ dq(W)^T (+ bias)
// x is bf16 (row stride xs >= K, unit column stride), W is an Fp8Pack read
// exactly as the weight-streaming decode kernels read it (common.cuh "FP8
// weight pack": fp8_pack_off, fp8x8_to_bf16x8), so a pack-resident fp8 model
// needs no bf16 copy of a projection for prefill, decode above 64 rows or
// the generic path.
//
// Work split.  A block of 4 waves owns a BM x BN = 128 x 128 output tile;
// the waves sit 2 x 2 on it, so a wave owns 64 rows x 64 columns: two
// 32-row M sub-tiles times two 32-column pack tiles, four 32x32 fp32
// accumulators.  No k split: every accumulator sums its whole K in
// ascending k, one mfma_f32_32x32x16_bf16 per 16 k.
//
// B (weights) never touches LDS.  The pack is already in MFMA fragment
// order: for pack tile t and k-block b a lane's two 16-byte units are
// ((t*NB + b)*2 + jj)*64 + lane, and unit jj carries the lane's fragments
// 2*jj (.xy) and 2*jj + 1 (.zw).  A wave loads its 2 tiles x 2 units with
// dwordx4, widens each fragment to bf16 once (exact) and uses it for both
// of its M sub-tiles.
//
// A (activations) is staged: the block's 128 x 64 bf16 x tile goes from
// global memory (coalesced 16-byte chunks, 128 B per row, rows clamped to
// M - 1 so row M is never read) into a 16 KiB LDS tile, 16-byte unit
// r*8 + (c ^ (r & 7)): the 8 chunks of a row are rotated by the row so the
// fragment reads (32 rows, one chunk column) spread over all banks.  Two
// such tiles double-buffer k: while the MFMAs of k-block b issue, the x
// chunks and the B codes of block b + 1 are already in flight to registers;
// the x chunks are written to the other tile after the MFMAs and ONE
// barrier per k-block publishes them.
//
// Epilogue.  acc * scale[pack row] in fp32 (a power of two: commutes with
// every rounding), + bias, one rounding to bf16, written to an LDS output
// tile (it aliases the x tiles; the loop's last barrier has closed them),
// then stored as 16-byte row-contiguous chunks:
//   mode 0 plain  y[m, t*32 + r]
//   mode 1 qkv    y[m, colmap[t*32 + r]]: the pair order of the fused RoPE
//                 pack keeps runs of 16 natural columns together, so every
//                 aligned 8-column chunk of a pack tile is 8 consecutive
//                 natural columns; the bias is in natural order
//   mode 2 gu     tile t = 16 gate rows then their 16 up rows: the up value
//                 comes over from lane + 16, act = silu(g) * u in fp32 from
//                 the scaled accumulators, y is [M, N/2]; the [M, N]
//                 intermediate never exists
// Rows >= M and pack tiles >= N/32 (a partial last N block) are computed on
// clamped addresses and never stored.  All global offsets are 64-bit.
#include "common.cuh"
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int W8_BM = 128, W8_BN = 128;
constexpr int W8_THREADS = 256;
constexpr int W8_XTILE = W8_BM * 64;            // bf16 elements, one k-block
constexpr int W8_OPITCH = W8_BN + 8;            // output tile row, bf16
constexpr int W8_LDS = W8_BM * W8_OPITCH * 2;   // 34816 B >= two x tiles
static_assert(W8_LDS >= 2 * W8_XTILE * 2, "output tile must cover x tiles");

enum { W8_PLAIN = 0, W8_QKV = 1, W8_GU = 2 };

template <int MODE>
__global__ __launch_bounds__(W8_THREADS) void k_w8_gemm(
    bf16* __restrict__ y,              // [M, N] or [M, N/2] (gu), dense
    const bf16* __restrict__ x,        // [M, K], row stride xs
    const u32x4* __restrict__ wp,      // fp8 pack codes
    const float* __restrict__ wscale,  // [N] pack row order
    const bf16* __restrict__ bias,     // [N] natural order, or null
    const int* __restrict__ colmap,    // [N] natural column of a pack column
    int M, int N, int K, int64_t xs)
{
    __shared__ __align__(16) char smem[W8_LDS];
    const int tid = threadIdx.x;
    const int wid = tid >> 6, lane = tid & 63;
    const int wm = wid >> 1, wn = wid & 1;
    const int row = lane & 31, h = lane >> 5;
    const int NB = K >> 6, NT = N >> 5;
    const int m0 = blockIdx.y * W8_BM;
    const int tb = blockIdx.x * (W8_BN / 32);   // block's first pack tile
    const int t0 = tb + wn * 2;                 // wave's first pack tile
    // a wave whose 64 rows all lie past M only stages x and keeps barriers
    const bool live = m0 + wm * 64 < M;

    // x staging: thread -> chunk c of rows sr + 32*i
    const int sc = tid & 7, sr = tid >> 3;
    const bf16* xg[4];
    int xu[4];                                   // LDS unit of each chunk
    #pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = sr + 32 * i;
        const int gm = m0 + r < M ? m0 + r : M - 1;
        xg[i] = x + (int64_t)gm * xs + sc * 8;
        xu[i] = r * 8 + (sc ^ (r & 7));
    }
    // B: clamped tile ids keep a dead tile's loads inside the pack
    const u32x4* wb[2];
    #pragma unroll
    for (int i = 0; i < 2; i++) {
        const int t = t0 + i < NT ? t0 + i : NT - 1;
        wb[i] = wp + (int64_t)t * NB * 128 + lane;
    }
    // A fragment units: sub-tile ms, fragment j -> chunk j*2 + h of row ra
    int au[2][4];
    #pragma unroll
    for (int ms = 0; ms < 2; ms++) {
        const int ra = wm * 64 + ms * 32 + row;
        #pragma unroll
        for (int j = 0; j < 4; j++)
            au[ms][j] = ra * 8 + ((j * 2 + h) ^ (ra & 7));
    }

    u32x4* xt = reinterpret_cast<u32x4*>(smem);      // [2][1024] units
    u32x4 xr[4];
    u32x4 bq[2][2][2];                           // [ring slot][tile][unit]
    f32x16 acc[2][2] = {};

    auto load_x = [&](int b) {
        #pragma unroll
        for (int i = 0; i < 4; i++)
            xr[i] = *reinterpret_cast<const u32x4*>(
                xg[i] + ((int64_t)b << 6));
    };
    auto store_x = [&](int s) {
        #pragma unroll
        for (int i = 0; i < 4; i++)
            xt[s * 1024 + xu[i]] = xr[i];
    };
    auto load_b = [&](auto S, int b) {           // into ring slot S
        constexpr int s = decltype(S)::value;
        #pragma unroll
        for (int i = 0; i < 2; i++) {
            const u32x4* q = wb[i] + (int64_t)b * 128;
            bq[s][i][0] = q[0];
            bq[s][i][1] = q[64];
        }
    };
    // k-block b from x tile / B slot S = b & 1; prefetches block b + 1
    auto step = [&](auto S, int b) {
        constexpr int s = decltype(S)::value;
        const bool more = b + 1 < NB;
        if (more) {
            load_x(b + 1);
            if (live) load_b(std::integral_constant<int, s ^ 1>{}, b + 1);
        }
        if (live) {
            bf16x8 a[2][4];
            #pragma unroll
            for (int ms = 0; ms < 2; ms++)
                #pragma unroll
                for (int j = 0; j < 4; j++)
                    a[ms][j] = __builtin_bit_cast(
                        bf16x8, xt[s * 1024 + au[ms][j]]);
            #pragma unroll
            for (int i = 0; i < 2; i++) {
                bf16x8 vb[4];
                vb[0] = fp8x8_to_bf16x8(bq[s][i][0].x, bq[s][i][0].y);
                vb[1] = fp8x8_to_bf16x8(bq[s][i][0].z, bq[s][i][0].w);
                vb[2] = fp8x8_to_bf16x8(bq[s][i][1].x, bq[s][i][1].y);
                vb[3] = fp8x8_to_bf16x8(bq[s][i][1].z, bq[s][i][1].w);
                #pragma unroll
                for (int ms = 0; ms < 2; ms++)
                    #pragma unroll
                    for (int j = 0; j < 4; j++)
                        acc[ms][i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            a[ms][j], vb[j], acc[ms][i], 0, 0, 0);
            }
        }
        if (more) store_x(s ^ 1);
        __syncthreads();
    };

    load_x(0);
    if (live) load_b(std::integral_constant<int, 0>{}, 0);
    store_x(0);
    __syncthreads();
    for (int b = 0; b < NB; b += 2) {
        step(std::integral_constant<int, 0>{}, b);
        if (b + 1 < NB) step(std::integral_constant<int, 1>{}, b + 1);
    }

    // ---- epilogue: scale, bias / SwiGLU, round once, stage, store ----
    constexpr int OW = MODE == W8_GU ? 16 : 32;   // y columns per pack tile
    bf16* ot = reinterpret_cast<bf16*>(smem);
    if (live) {
        #pragma unroll
        for (int i = 0; i < 2; i++) {
            if (t0 + i >= NT) continue;           // wave-uniform
            const int pc = (t0 + i) * 32 + row;   // pack column
            const float scl = wscale[pc];
            float bv = 0.f;
            if (MODE != W8_GU && bias)
                bv = bf2f(bias[MODE == W8_QKV ? colmap[pc] : pc]);
            #pragma unroll
            for (int ms = 0; ms < 2; ms++) {
                #pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int lr = wm * 64 + ms * 32
                                   + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float v = acc[ms][i][r] * scl;
                    if (MODE == W8_GU) {
                        const float u = __shfl_xor(v, 16, 64);
                        if (row < 16)
                            ot[lr * W8_OPITCH + (wn * 2 + i) * OW + row] =
                                f2bf((v / (1.f + __expf(-v))) * u);
                    } else {
                        ot[lr * W8_OPITCH + (wn * 2 + i) * OW + row] =
                            f2bf(v + bv);
                    }
                }
            }
        }
    }
    __syncthreads();
    constexpr int CPT = OW / 8;                   // 16-byte chunks per tile
    constexpr int CPR = (W8_BN / 32) * CPT;       // and per block row
    const int64_t ys = MODE == W8_GU ? (N >> 1) : N;
    for (int idx = tid; idx < W8_BM * CPR; idx += W8_THREADS) {
        const int lr = idx / CPR, ch = idx % CPR;
        const int ti = ch / CPT, cc = ch % CPT;
        const int gm = m0 + lr, t = tb + ti;
        if (gm >= M || t >= NT) continue;
        const int col = MODE == W8_QKV ? colmap[t * 32 + cc * 8]
                                       : t * OW + cc * 8;
        *reinterpret_cast<u32x4*>(y + (int64_t)gm * ys + col) =
            *reinterpret_cast<const u32x4*>(
                ot + lr * W8_OPITCH + ti * OW + cc * 8);
    }
}

}  // namespace

// mode: 0 plain, 1 qkv (colmap required), 2 gu (no bias; y is [M, N/2]).
extern "C" int w8_gemm_bf16(void* y, const void* x, const void* codes,
                            const void* scale, const void* bias,
                            const void* colmap, int M, int N, int K,
                            int64_t xs, int mode, void* stream_) {
    if (!y || !x || !codes || !scale || M < 1 || N < 32 || N % 32
            || K < 64 || K % 64 || xs < K || xs % 8
            || mode < W8_PLAIN || mode > W8_GU
            || (mode == W8_QKV && !colmap) || (mode == W8_GU && bias))
        return (int)hipErrorInvalidValue;
    const int64_t mblocks = ((int64_t)M + W8_BM - 1) / W8_BM;
    if (mblocks > 65535) return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    dim3 grid((N / 32 + W8_BN / 32 - 1) / (W8_BN / 32), (unsigned)mblocks);
#define W8_LAUNCH(MODE)                                                     \
    k_w8_gemm<MODE><<<grid, W8_THREADS, 0, stream>>>(                       \
        (bf16*)y, (const bf16*)x, (const u32x4*)codes, (const float*)scale, \
        (const bf16*)bias, (const int*)colmap, M, N, K, xs)
    if (mode == W8_QKV) W8_LAUNCH(W8_QKV);
    else if (mode == W8_GU) W8_LAUNCH(W8_GU);
    else W8_LAUNCH(W8_PLAIN);
#undef W8_LAUNCH
    return (int)hipGetLastError();
}
