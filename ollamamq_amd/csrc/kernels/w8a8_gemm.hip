// W8A8 prefill for pack-resident fp8 models: a per-token activation
// quantiser and an MFMA GEMM that multiplies fp8 activations by an Fp8Pack
// with the native fp8 matrix instruction (v_mfma_f32_32x32x64_f8f6f4).
//
//   act_quant_fp8   x bf16 [M, K] -> codes e4m3fn [M, K], exps int32 [M]
//   w8a8_gemm_bf16  y[M, N] = (dq(xq) @ dq(W)^T) (+ bias), bf16 out
//
// ---- quantiser ----
// Row m is ops/quant.py quantize_fp8 of that row: e = ceil(log2(absmax /
// 448)) by the frexp rule (all-zero row: 0), q = e4m3fn(x * 2^-e) rounded to
// nearest even.  One block per row.  A thread keeps up to AQ_REG 16-byte
// chunks of the row in registers (K <= 32768 is read once; the chunks past
// that are read a second time).  absmax is an integer max over the bf16
// magnitude bits (wave reduce, one LDS step), the exponent comes from the
// bit fields of that maximum, and a code is encoded from the top 16 bits of
// x * 2^-e (v_ldexp_f32) by the integer encoder the KV cache uses
// (common.cuh bf16_to_e4m3).  A product of 2^-126 or more keeps x's
// mantissa and is exactly a bf16 value; a smaller one is an fp32 denormal,
// whose top 16 bits have exponent field 0 whether or not it is flushed, and
// everything under 2^-10 encodes to the signed zero anyway.  A bf16
// subnormal INPUT is an fp32 denormal too: it is scaled correctly because
// the kernel is compiled with fp32 denormals kept (hipcc's default here);
// it matters only for a row whose maximum is itself under 2^-107.
// Nothing is indexed by data.
//
// ---- GEMM ----
// Work split as w8_gemm.hip: a block of 4 waves owns 128 x 128 outputs, the
// waves sit 2 x 2, a wave owns two 32-row M sub-tiles times two pack tiles,
// four 32x32 fp32 accumulators, no k split, ascending k.
//
// B never touches LDS and is never converted.  For pack tile t and k-block b
// a lane's two 16-byte units ((t*NB + b)*2 + jj)*64 + lane hold its codes
// for k = b*64 + j*16 + h*8 + e in [j][e] order (h = lane >> 5): the two
// units concatenated ARE the 8-dword B operand of one 32x32x64 MFMA.  The
// instruction sums over k, and its A and B operands map (lane half, byte)
// to k the same way, so A only has to hold the same k at the same byte.
//
// A is staged.  A barrier step covers W8A8_KS = 128 k (two k-blocks): the
// block's 128 rows x 128 code bytes go from global memory (16-byte chunks,
// 128 B per row per instruction, rows clamped to M - 1) to a 16 KiB LDS
// tile.  Natural chunk c of a row is k-block kb = c >> 2, fragment j = c & 3,
// with half 0 in its low and half 1 in its high 8 bytes; the staging write
// puts them at [kb][h][j][e], so a lane of half h reads its 32 bytes of a
// k-block as two ds_read_b128.  Unit r*8 + (u ^ (r & 7)) rotates a row's 8
// units by the row.  Two tiles double-buffer k: the x chunks and the B units
// of step s + 1 are in flight to registers while the 8 MFMAs of step s
// issue; one barrier per step.  A last half step (K % 128 == 64) loads
// clamped addresses and skips its second k-block's MFMAs.
//
// Epilogue as w8_gemm.hip with one more exact factor: acc * scale[pack row]
// in fp32, ldexp by the row's activation exponent (both powers of two), +
// bias, one rounding to bf16, staged through LDS, 16-byte row-contiguous
// stores; modes plain / qkv (colmap) / gu (fused SwiGLU, [M, N/2] out).
#include "common.cuh"
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

// ---------------------------------------------------------------------------
constexpr int AQ_THREADS = 256;
constexpr int AQ_REG = 16;      // 16-byte chunks a thread keeps in registers

DEV unsigned absmax4(unsigned m, const u32x4 v) {
    #pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned lo = v[i] & 0x7fffu, hi = (v[i] >> 16) & 0x7fffu;
        m = m > lo ? m : lo;
        m = m > hi ? m : hi;
    }
    return m;
}

// one bf16 (low 16 bits of b) times 2^-e -> e4m3fn code
DEV unsigned quant1(unsigned b, int e) {
    const float s = ldexpf(__uint_as_float(b << 16), -e);
    return bf16_to_e4m3(__float_as_uint(s) >> 16);
}

DEV uint2 quant8(const u32x4 v, int e) {
    unsigned c[4];
    #pragma unroll
    for (int i = 0; i < 4; i++)
        c[i] = quant1(v[i] & 0xffffu, e) | (quant1(v[i] >> 16, e) << 8);
    return make_uint2(c[0] | (c[1] << 16), c[2] | (c[3] << 16));
}

__global__ __launch_bounds__(AQ_THREADS) void k_act_quant_fp8(
    uint8_t* __restrict__ codes,       // [M, K] dense
    int* __restrict__ exps,            // [M]
    const bf16* __restrict__ x,        // [M, K], row stride xs
    int K, int64_t xs)
{
    __shared__ unsigned wmax[AQ_THREADS / 64];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    const u32x4* xr = reinterpret_cast<const u32x4*>(x + m * xs);
    uint2* cr = reinterpret_cast<uint2*>(codes + m * K);
    const int NC = K >> 3;                       // 16-byte chunks of the row

    u32x4 v[AQ_REG];
    unsigned amax = 0;
    #pragma unroll
    for (int i = 0; i < AQ_REG; i++) {
        const int c = tid + i * AQ_THREADS;
        v[i] = c < NC ? xr[c] : u32x4{0, 0, 0, 0};
        amax = absmax4(amax, v[i]);
    }
    for (int c = tid + AQ_REG * AQ_THREADS; c < NC; c += AQ_THREADS)
        amax = absmax4(amax, xr[c]);
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(amax, off, 64);
        amax = amax > o ? amax : o;
    }
    if ((tid & 63) == 0) wmax[tid >> 6] = amax;
    __syncthreads();
    #pragma unroll
    for (int w = 0; w < AQ_THREADS / 64; w++)
        amax = amax > wmax[w] ? amax : wmax[w];

    // amax = (1 + f/128) * 2^(E - 127): frexp's x is E - 126 and its
    // m > 0.875 <=> f > 96, so e = x - 9 + (m > 0.875) = E - 135 + (f > 96)
    int E = (int)(amax >> 7);
    unsigned f = amax & 0x7fu;
    if (E == 0 && f) {                           // bf16 subnormal: normalise
        const int p = 31 - __clz((int)f);        // 0..6
        f = (f << (7 - p)) & 0x7fu;
        E = p - 6;
    }
    const int e = amax ? E - 135 + (f > 96u ? 1 : 0) : 0;
    if (tid == 0) exps[m] = e;

    #pragma unroll
    for (int i = 0; i < AQ_REG; i++) {
        const int c = tid + i * AQ_THREADS;
        if (c < NC) cr[c] = quant8(v[i], e);
    }
    for (int c = tid + AQ_REG * AQ_THREADS; c < NC; c += AQ_THREADS)
        cr[c] = quant8(xr[c], e);
}

// ---------------------------------------------------------------------------
constexpr int W8A8_BM = 128, W8A8_BN = 128;
constexpr int W8A8_THREADS = 256;
constexpr int W8A8_XUNITS = W8A8_BM * 8;          // 16-byte units, one step
constexpr int W8A8_OPITCH = W8A8_BN + 8;          // output tile row, bf16
constexpr int W8A8_LDS = W8A8_BM * W8A8_OPITCH * 2;   // 34816 B
static_assert(W8A8_LDS >= 2 * W8A8_XUNITS * 16, "output tile covers x tiles");

enum { W8A8_PLAIN = 0, W8A8_QKV = 1, W8A8_GU = 2 };

template <int MODE>
__global__ __launch_bounds__(W8A8_THREADS) void k_w8a8_gemm(
    bf16* __restrict__ y,              // [M, N] or [M, N/2] (gu), dense
    const uint8_t* __restrict__ xq,    // [M, K] e4m3fn codes, dense
    const int* __restrict__ xexp,      // [M] activation row exponents
    const u32x4* __restrict__ wp,      // fp8 pack codes
    const float* __restrict__ wscale,  // [N] pack row order
    const bf16* __restrict__ bias,     // [N] natural order, or null
    const int* __restrict__ colmap,    // [N] natural column of a pack column
    int M, int N, int K)
{
    __shared__ __align__(16) char smem[W8A8_LDS];
    __shared__ int sxe[W8A8_BM];
    const int tid = threadIdx.x;
    const int wid = tid >> 6, lane = tid & 63;
    const int wm = wid >> 1, wn = wid & 1;
    const int row = lane & 31, h = lane >> 5;
    const int NB = K >> 6, NT = N >> 5;
    const int NS = (NB + 1) >> 1;                // barrier steps
    const int m0 = blockIdx.y * W8A8_BM;
    const int tb = blockIdx.x * (W8A8_BN / 32);  // block's first pack tile
    const int t0 = tb + wn * 2;                  // wave's first pack tile
    // a wave whose 64 rows all lie past M only stages x and keeps barriers
    const bool live = m0 + wm * 64 < M;

    if (tid < W8A8_BM)
        sxe[tid] = xexp[m0 + tid < M ? m0 + tid : M - 1];

    // x staging: thread -> natural chunk sc (16 codes) of rows sr + 32*i;
    // its low 8 bytes go to half 0, its high 8 bytes to half 1
    const int sc = tid & 7, sr = tid >> 3;
    const int skb = sc >> 2, sj = sc & 3;
    const uint8_t* xg[4];
    int xo[4];                                   // LDS byte offset, half 0
    #pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = sr + 32 * i;
        const int gm = m0 + r < M ? m0 + r : M - 1;
        xg[i] = xq + (int64_t)gm * K + sc * 16;
        const int u = skb * 4 + (sj >> 1);       // unit of half 0; half 1: +2
        xo[i] = (r * 8 + (u ^ (r & 7))) * 16 + (sj & 1) * 8;
    }
    // half 1 sits two units on: (u + 2) ^ (r & 7) = (u ^ (r & 7)) ^ 2
    // B: clamped tile ids keep a dead tile's loads inside the pack
    const u32x4* wb[2];
    #pragma unroll
    for (int i = 0; i < 2; i++) {
        const int t = t0 + i < NT ? t0 + i : NT - 1;
        wb[i] = wp + (int64_t)t * NB * 128 + lane;
    }
    // A operand units: sub-tile ms, k-block kb of the step -> units
    // kb*4 + h*2 + {0, 1} of row ra
    int au[2][2][2];
    #pragma unroll
    for (int ms = 0; ms < 2; ms++) {
        const int ra = wm * 64 + ms * 32 + row;
        #pragma unroll
        for (int kb = 0; kb < 2; kb++)
            #pragma unroll
            for (int q = 0; q < 2; q++)
                au[ms][kb][q] = ra * 8 + ((kb * 4 + h * 2 + q) ^ (ra & 7));
    }

    u32x4* xt = reinterpret_cast<u32x4*>(smem);      // [2][1024] units
    u32x4 xr[4];
    u32x4 bq[2][2][2][2];                // [ring slot][k-block][tile][unit]
    f32x16 acc[2][2] = {};

    // a half last step re-reads its first k-block instead of running past K
    auto load_x = [&](int s) {
        const bool half = skb && 2 * s + 1 >= NB;
        const int64_t off = ((int64_t)s << 7) - (half ? 64 : 0);
        #pragma unroll
        for (int i = 0; i < 4; i++)
            xr[i] = *reinterpret_cast<const u32x4*>(xg[i] + off);
    };
    auto store_x = [&](int s) {
        char* base = smem + s * (W8A8_XUNITS * 16);
        #pragma unroll
        for (int i = 0; i < 4; i++) {
            *reinterpret_cast<uint2*>(base + xo[i]) =
                make_uint2(xr[i].x, xr[i].y);
            *reinterpret_cast<uint2*>(base + (xo[i] ^ 32)) =
                make_uint2(xr[i].z, xr[i].w);
        }
    };
    auto load_b = [&](auto S, int s) {           // into ring slot S
        constexpr int sl = decltype(S)::value;
        #pragma unroll
        for (int kb = 0; kb < 2; kb++) {
            const int b = 2 * s + kb < NB ? 2 * s + kb : NB - 1;
            #pragma unroll
            for (int i = 0; i < 2; i++) {
                const u32x4* q = wb[i] + (int64_t)b * 128;
                bq[sl][kb][i][0] = q[0];
                bq[sl][kb][i][1] = q[64];
            }
        }
    };
    // step s from x tile / B slot S = s & 1; prefetches step s + 1
    auto step = [&](auto S, int s) {
        constexpr int sl = decltype(S)::value;
        const bool more = s + 1 < NS;
        if (more) {
            load_x(s + 1);
            if (live) load_b(std::integral_constant<int, sl ^ 1>{}, s + 1);
        }
        if (live) {
            #pragma unroll
            for (int kb = 0; kb < 2; kb++) {
                if (kb && 2 * s + 1 >= NB) break;        // block-uniform
                i32x8 a[2];
                #pragma unroll
                for (int ms = 0; ms < 2; ms++) {
                    const u32x4 lo = xt[sl * W8A8_XUNITS + au[ms][kb][0]];
                    const u32x4 hi = xt[sl * W8A8_XUNITS + au[ms][kb][1]];
                    a[ms] = i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w,
                                  (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
                }
                #pragma unroll
                for (int i = 0; i < 2; i++) {
                    const u32x4 lo = bq[sl][kb][i][0], hi = bq[sl][kb][i][1];
                    const i32x8 vb = {(int)lo.x, (int)lo.y, (int)lo.z,
                                      (int)lo.w, (int)hi.x, (int)hi.y,
                                      (int)hi.z, (int)hi.w};
                    #pragma unroll
                    for (int ms = 0; ms < 2; ms++)
                        acc[ms][i] =
                            __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                                a[ms], vb, acc[ms][i], 0, 0, 0, 0, 0, 0);
                }
            }
        }
        if (more) store_x(sl ^ 1);
        __syncthreads();
    };

    load_x(0);
    if (live) load_b(std::integral_constant<int, 0>{}, 0);
    store_x(0);
    __syncthreads();
    for (int s = 0; s < NS; s += 2) {
        step(std::integral_constant<int, 0>{}, s);
        if (s + 1 < NS) step(std::integral_constant<int, 1>{}, s + 1);
    }

    // ---- epilogue: scales, bias / SwiGLU, round once, stage, store ----
    constexpr int OW = MODE == W8A8_GU ? 16 : 32;  // y columns per pack tile
    bf16* ot = reinterpret_cast<bf16*>(smem);
    if (live) {
        #pragma unroll
        for (int i = 0; i < 2; i++) {
            if (t0 + i >= NT) continue;           // wave-uniform
            const int pc = (t0 + i) * 32 + row;   // pack column
            const float scl = wscale[pc];
            float bv = 0.f;
            if (MODE != W8A8_GU && bias)
                bv = bf2f(bias[MODE == W8A8_QKV ? colmap[pc] : pc]);
            #pragma unroll
            for (int ms = 0; ms < 2; ms++) {
                #pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int lr = wm * 64 + ms * 32
                                   + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const float v = ldexpf(acc[ms][i][r] * scl, sxe[lr]);
                    if (MODE == W8A8_GU) {
                        const float u = __shfl_xor(v, 16, 64);
                        if (row < 16)
                            ot[lr * W8A8_OPITCH + (wn * 2 + i) * OW + row] =
                                f2bf((v / (1.f + __expf(-v))) * u);
                    } else {
                        ot[lr * W8A8_OPITCH + (wn * 2 + i) * OW + row] =
                            f2bf(v + bv);
                    }
                }
            }
        }
    }
    __syncthreads();
    constexpr int CPT = OW / 8;                   // 16-byte chunks per tile
    constexpr int CPR = (W8A8_BN / 32) * CPT;     // and per block row
    const int64_t ys = MODE == W8A8_GU ? (N >> 1) : N;
    for (int idx = tid; idx < W8A8_BM * CPR; idx += W8A8_THREADS) {
        const int lr = idx / CPR, ch = idx % CPR;
        const int ti = ch / CPT, cc = ch % CPT;
        const int gm = m0 + lr, t = tb + ti;
        if (gm >= M || t >= NT) continue;
        const int col = MODE == W8A8_QKV ? colmap[t * 32 + cc * 8]
                                         : t * OW + cc * 8;
        *reinterpret_cast<u32x4*>(y + (int64_t)gm * ys + col) =
            *reinterpret_cast<const u32x4*>(
                ot + lr * W8A8_OPITCH + ti * OW + cc * 8);
    }
}

}  // namespace

extern "C" int act_quant_fp8(void* codes, void* exps, const void* x,
                             int M, int K, int64_t xs, void* stream_) {
    if (!codes || !exps || !x || M < 1 || K < 8 || K % 8 || xs < K || xs % 8)
        return (int)hipErrorInvalidValue;
    k_act_quant_fp8<<<(unsigned)M, AQ_THREADS, 0, (hipStream_t)stream_>>>(
        (uint8_t*)codes, (int*)exps, (const bf16*)x, K, xs);
    return (int)hipGetLastError();
}

// mode: 0 plain, 1 qkv (colmap required), 2 gu (no bias; y is [M, N/2]).
extern "C" int w8a8_gemm_bf16(void* y, const void* xq, const void* xexp,
                              const void* codes, const void* scale,
                              const void* bias, const void* colmap,
                              int M, int N, int K, int mode, void* stream_) {
    if (!y || !xq || !xexp || !codes || !scale || M < 1 || N < 32 || N % 32
            || K < 64 || K % 64 || mode < W8A8_PLAIN || mode > W8A8_GU
            || (mode == W8A8_QKV && !colmap) || (mode == W8A8_GU && bias))
        return (int)hipErrorInvalidValue;
    const int64_t mblocks = ((int64_t)M + W8A8_BM - 1) / W8A8_BM;
    if (mblocks > 65535) return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    dim3 grid((N / 32 + W8A8_BN / 32 - 1) / (W8A8_BN / 32),
              (unsigned)mblocks);
#define W8A8_LAUNCH(MODE)                                                   \
    k_w8a8_gemm<MODE><<<grid, W8A8_THREADS, 0, stream>>>(                   \
        (bf16*)y, (const uint8_t*)xq, (const int*)xexp,                     \
        (const u32x4*)codes, (const float*)scale, (const bf16*)bias,        \
        (const int*)colmap, M, N, K)
    if (mode == W8A8_QKV) W8A8_LAUNCH(W8A8_QKV);
    else if (mode == W8A8_GU) W8A8_LAUNCH(W8A8_GU);
    else W8A8_LAUNCH(W8A8_PLAIN);
#undef W8A8_LAUNCH
    return (int)hipGetLastError();
}
