// gfx950 (MI355X / CDNA4) inference kernels for ollamamq_amd.
//
// Hand-written HIP for the hot ops the reference delegates to external
// Ollama backends (the reference has zero GPU code; this is
// new construction mandated by the north star): fused residual+RMSNorm,
// RoPE, paged-KV append, paged decode/prefill attention with LDS-staged KV
// tiles, SwiGLU, greedy sampler.
//
// Conventions (cdna_hip_programming.md):
//  * wave = 64 lanes, block sizes are multiples of 64;
//  * bf16 I/O, fp32 math; vectorized 16B loads (G13);
//  * LDS rows padded to kill bank conflicts (G4);
//  * no CUDA-compat shims; compiled only for --offload-arch=gfx950.
//
// Exposed as extern "C" launchers taking raw device pointers + hipStream_t,
// bound from Python via ctypes (ops/hip.py) — no torch ABI dependency.

#include "common.cuh"

DEV void store8bf(bf16* p, const float* in) {
    bf162* v = reinterpret_cast<bf162*>(p);
    v[0] = __float22bfloat162_rn(make_float2(in[0], in[1]));
    v[1] = __float22bfloat162_rn(make_float2(in[2], in[3]));
    v[2] = __float22bfloat162_rn(make_float2(in[4], in[5]));
    v[3] = __float22bfloat162_rn(make_float2(in[6], in[7]));
}

// ---------------------------------------------------------------------------
// Fused residual-add + RMSNorm.  y = rmsnorm(x + res) * w;  res_out = x + res.
// One 256-thread block per row; H multiple of 8; bf16 x8 vectorized.
// Memory-bound: reads x(+res)+w, writes y(+res_out) — single pass.
// ---------------------------------------------------------------------------
// VPT = 8-element vectors per thread (ceil(H / 2048)); the whole row
// stays in registers between the reduce and the scale, so each block does
// ONE read of x(+res) and one write each of res_out and y — the two-pass
// version re-read its own store and its second pass re-paid load latency
// (decode rows are few: the grid is tiny and latency-bound).
template <int VPT, bool EXACT>   // EXACT: H == VPT*2048, no tail guards
__global__ __launch_bounds__(256) void k_rmsnorm_residual(
    bf16* __restrict__ y, bf16* __restrict__ res_out,
    const bf16* __restrict__ x, const bf16* __restrict__ res_in,
    const bf16* __restrict__ w, int H, float eps)
{
    const int row = blockIdx.x;
    const bf16* xr = x + (int64_t)row * H;
    const bf16* rr = res_in ? res_in + (int64_t)row * H : nullptr;
    bf16* yr = y + (int64_t)row * H;
    bf16* ro = res_out + (int64_t)row * H;

    float v[VPT][8];
    float ss = 0.f;
    #pragma unroll
    for (int u = 0; u < VPT; u++) {
        const int i = threadIdx.x * 8 + u * 2048;
        if (EXACT || i < H) {
            load8f(xr + i, v[u]);
            if (rr) {
                float vr[8];
                load8f(rr + i, vr);
                #pragma unroll
                for (int j = 0; j < 8; j++) v[u][j] += vr[j];
            }
            #pragma unroll
            for (int j = 0; j < 8; j++) ss += v[u][j] * v[u][j];
            store8bf(ro + i, v[u]);
        }
    }
    ss = wave_reduce_sum(ss);
    __shared__ float warp_ss[4];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) warp_ss[wid] = ss;
    __syncthreads();
    float tot = warp_ss[0] + warp_ss[1] + warp_ss[2] + warp_ss[3];
    const float inv = rsqrtf(tot / H + eps);

    #pragma unroll
    for (int u = 0; u < VPT; u++) {
        const int i = threadIdx.x * 8 + u * 2048;
        if (EXACT || i < H) {
            float vw[8];
            load8f(w + i, vw);
            #pragma unroll
            for (int j = 0; j < 8; j++) v[u][j] = v[u][j] * inv * vw[j];
            store8bf(yr + i, v[u]);
        }
    }
}

extern "C" int rmsnorm_residual_bf16(
    void* y, void* res_out, const void* x, const void* res_in,
    const void* w, int T, int H, float eps, hipStream_t stream)
{
    // EXACT sizes skip the per-vector guard: a runtime `i < H` around
    // loads de-pipelines them (guide §5 traps (c)); every model hidden
    // size here is a multiple of 2048 except the tiny test presets.
    #define RMS_LAUNCH(VPT, EX)                                           \
        k_rmsnorm_residual<VPT, EX><<<T, 256, 0, stream>>>(               \
            (bf16*)y, (bf16*)res_out, (const bf16*)x,                     \
            (const bf16*)res_in, (const bf16*)w, H, eps)
    if (H == 2048) RMS_LAUNCH(1, true);
    else if (H == 4096) RMS_LAUNCH(2, true);
    else if (H == 8192) RMS_LAUNCH(4, true);
    else if (H == 16384) RMS_LAUNCH(8, true);
    else if (H <= 2048) RMS_LAUNCH(1, false);
    else if (H <= 4096) RMS_LAUNCH(2, false);
    else if (H <= 8192) RMS_LAUNCH(4, false);
    else if (H <= 16384) RMS_LAUNCH(8, false);
    else return (int)hipErrorInvalidValue;
    #undef RMS_LAUNCH
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// RoPE (NeoX half-rotation), in place on q [T,Hq,D] and k [T,Hk,D], D=128.
// cos/sin: [max_ctx, D/2] fp32 host-precomputed (Appendix B: no device trig).
// One wave per (token, head); lane l rotates dims (l, l+64).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rope(
    bf16* __restrict__ q, bf16* __restrict__ k,
    const int* __restrict__ pos, const float* __restrict__ cost,
    const float* __restrict__ sint, int T, int Hq, int Hk, int D,
    int64_t qs, int64_t ks)   // row strides in elements (fused-QKV views)
{
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);  // (token,head) flat
    const int lane = threadIdx.x & 63;
    const int Htot = Hq + Hk;
    if (gid >= T * Htot) return;
    const int t = gid / Htot, h = gid % Htot;
    bf16* base = (h < Hq) ? q + (int64_t)t * qs + (int64_t)h * D
                          : k + (int64_t)t * ks + (int64_t)(h - Hq) * D;
    const int d2 = D / 2;                 // 64 = one lane per rotation pair
    const float c = cost[(int64_t)pos[t] * d2 + lane];
    const float s = sint[(int64_t)pos[t] * d2 + lane];
    const float x1 = bf2f(base[lane]);
    const float x2 = bf2f(base[lane + d2]);
    base[lane] = f2bf(x1 * c - x2 * s);
    base[lane + d2] = f2bf(x2 * c + x1 * s);
}

extern "C" int rope_bf16(
    void* q, void* k, const void* pos, const void* cost, const void* sint,
    int T, int Hq, int Hk, int D, int64_t qs, int64_t ks,
    hipStream_t stream)
{
    const int waves = T * (Hq + Hk);
    k_rope<<<(waves + 3) / 4, 256, 0, stream>>>(
        (bf16*)q, (bf16*)k, (const int*)pos, (const float*)cost,
        (const float*)sint, T, Hq, Hk, D, qs, ks);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Paged-KV append: scatter k/v [T,KVH,D] to pool[layer] at (slot,pos).
// Pool layout and addressing: common.cuh paged_kv_row.  One wave per
// (token, head); lane moves 2 elems (D=128).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_kv_append(
    bf16* __restrict__ kp, bf16* __restrict__ vp,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const int* __restrict__ slot, const int* __restrict__ pos,
    const int* __restrict__ page_table,
    int T, int KVH, int D, int page, int max_pages, int64_t src_stride)
{
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gid >= T * KVH) return;
    const int t = gid / KVH, h = gid % KVH;
    const int64_t dst = paged_kv_row(page_table, slot[t], max_pages, pos[t],
                                     page, KVH, h);
    const int64_t src = (int64_t)t * src_stride + (int64_t)h * D;
    const bf162* ks = reinterpret_cast<const bf162*>(k + src);
    const bf162* vs = reinterpret_cast<const bf162*>(v + src);
    reinterpret_cast<bf162*>(kp + dst)[lane] = ks[lane];
    reinterpret_cast<bf162*>(vp + dst)[lane] = vs[lane];
}

extern "C" int kv_append_bf16(
    void* kp, void* vp, const void* k, const void* v, const void* slot,
    const void* pos, const void* page_table, int T, int KVH, int D,
    int page, int max_pages, int64_t src_stride, hipStream_t stream)
{
    const int waves = T * KVH;
    k_kv_append<<<(waves + 3) / 4, 256, 0, stream>>>(
        (bf16*)kp, (bf16*)vp, (const bf16*)k, (const bf16*)v,
        (const int*)slot, (const int*)pos, (const int*)page_table,
        T, KVH, D, page, max_pages, src_stride);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Paged attention, decode + prefill (flat varlen), D = 128, GQA group G ≤ 8.
// STATUS: legacy VALU path — superseded by decode_attn.hip
// (flash-decoding) and prefill_attn.hip (MFMA, 20x faster); kept as the
// OLLAMAMQ_VALU_PREFILL fallback and as the perf A/B baseline.
//
// Grid (n_tiles, KVH); block = G waves (one per q head in the group).
// Each tile covers QT query rows of one sequence.  KV is streamed in
// CHUNK=64-token tiles staged in LDS once per block and shared by the
// G q-heads (the GQA reuse is what makes this HBM-efficient: each KV byte
// is read once per kv-head, not once per q-head).
//
// LDS rows padded (+PAD bf16) so per-lane row reads are conflict-free
// (guide §6 G4: 256 B row stride = same-bank across all lanes).
//
// Decode instantiates QT=1 (one row per tile), prefill QT=16.
// Online softmax (m,l running, fp32), causal bound per query row.
// ---------------------------------------------------------------------------
#define CHUNK 64
#define DHEAD 128
#define KPAD 4     // bf16 elems of row padding

template <int QT>
__global__ __launch_bounds__(512) void k_paged_attn(
    bf16* __restrict__ out,           // [T, Hq, D]
    const bf16* __restrict__ q,       // [T, Hq, D]
    const bf16* __restrict__ kpool,   // [P][KVH][page][D]
    const bf16* __restrict__ vpool,
    const int* __restrict__ page_table,   // [slots][max_pages]
    const int* __restrict__ tile_slot,    // [n_tiles]
    const int* __restrict__ tile_q0,      // flat q row of tile start
    const int* __restrict__ tile_pos0,    // absolute position of tile start
    const int* __restrict__ tile_rows,    // rows in tile (≤ QT)
    int Hq, int KVH, int page, int max_pages, float scale, int64_t q_stride)
{
    const int tile = blockIdx.x;
    const int kvh = blockIdx.y;
    const int G = Hq / KVH;               // q heads per kv head (= waves)
    const int wid = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    if (wid >= G) return;                  // blockDim may exceed G*64
    const int qh = kvh * G + wid;

    const int slot = tile_slot[tile];
    const int q0 = tile_q0[tile];
    const int pos0 = tile_pos0[tile];
    const int rows = tile_rows[tile];
    const int kv_len = pos0 + rows;        // max kv any row may see

    // ---- LDS ----
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // k_tile [CHUNK][DHEAD+KPAD] bf16, v_tile same, q_lds [G][QT][DHEAD] f32?
    // q in fp32 would be 64KB at QT=16,G=8 — keep q bf16, widen on use.
    bf16* k_tile = reinterpret_cast<bf16*>(smem);
    const int KROW = DHEAD + KPAD;
    bf16* v_tile = k_tile + CHUNK * KROW;
    bf16* q_lds = v_tile + CHUNK * KROW;          // [G][QT][DHEAD]
    float* p_lds = reinterpret_cast<float*>(q_lds + (int64_t)G * QT * DHEAD);
    // p_lds [G][QT][CHUNK+1] f32
    const int PROW = CHUNK + 1;

    // ---- load this wave's Q rows into LDS (bf16, scaled later) ----
    for (int r = 0; r < rows; r++) {
        const bf16* qsrc = q + (int64_t)(q0 + r) * q_stride
                           + (int64_t)qh * DHEAD;
        reinterpret_cast<bf162*>(q_lds + ((int64_t)wid * QT + r) * DHEAD)[lane]
            = reinterpret_cast<const bf162*>(qsrc)[lane];
    }

    // ---- per-row online softmax state ----
    float m[QT], l[QT];
    // o accumulator: lane handles dims (2*lane, 2*lane+1) per row
    float o0[QT], o1[QT];
    #pragma unroll
    for (int r = 0; r < QT; r++) {
        m[r] = -3.0e38f; l[r] = 0.f; o0[r] = 0.f; o1[r] = 0.f;
    }
    __syncthreads();

    const int n_chunks = (kv_len + CHUNK - 1) / CHUNK;
    for (int ch = 0; ch < n_chunks; ch++) {
        const int base = ch * CHUNK;
        const int n_here = min(CHUNK, kv_len - base);
        // ---- stage K/V chunk (4 pages at page=16) into LDS, all threads --
        // Each (page,head) run in the pool is page*D contiguous bf16.
        __syncthreads();
        {
            const int tid = threadIdx.x, nthr = blockDim.x;
            const int total_vec = CHUNK * (DHEAD / 8);   // 16B units per tile
            for (int u = tid; u < total_vec; u += nthr) {
                const int tok = u / (DHEAD / 8);
                const int dv = u % (DHEAD / 8);
                if (base + tok < kv_len) {
                    const int64_t src =
                        paged_kv_row(page_table, slot, max_pages, base + tok,
                                     page, KVH, kvh) + dv * 8;
                    *reinterpret_cast<uint4*>(k_tile + tok * KROW + dv * 8) =
                        *reinterpret_cast<const uint4*>(kpool + src);
                    *reinterpret_cast<uint4*>(v_tile + tok * KROW + dv * 8) =
                        *reinterpret_cast<const uint4*>(vpool + src);
                }
            }
        }
        __syncthreads();

        // ---- scores: lane j owns key (base+j) ----
        const int j = lane;
        const bool live = j < n_here;
        float s[QT];
        #pragma unroll
        for (int r = 0; r < QT; r++) s[r] = 0.f;
        if (live) {
            const bf16* krow = k_tile + j * KROW;
            for (int d = 0; d < DHEAD; d += 8) {
                float kv8[8];
                load8f(krow + d, kv8);
                for (int r = 0; r < rows; r++) {
                    float q8[8];
                    load8f(q_lds + ((int64_t)wid * QT + r) * DHEAD + d, q8);
                    float acc = s[r];
                    #pragma unroll
                    for (int e = 0; e < 8; e++) acc += q8[e] * kv8[e];
                    s[r] = acc;
                }
            }
        }
        // causal mask + scale; dead lanes -inf
        for (int r = 0; r < rows; r++) {
            const int qpos = pos0 + r;
            const bool ok = live && (base + j <= qpos);
            s[r] = ok ? s[r] * scale : -3.0e38f;
        }

        // ---- online softmax update per row ----
        for (int r = 0; r < rows; r++) {
            const float smax = wave_reduce_max(s[r]);
            if (smax == -3.0e38f) {        // fully masked chunk for this row
                p_lds[((int64_t)wid * QT + r) * PROW + j] = 0.f;
                continue;
            }
            const float mn = fmaxf(m[r], smax);
            const float corr = __expf(m[r] - mn);
            const float p = (s[r] == -3.0e38f) ? 0.f : __expf(s[r] - mn);
            const float psum = wave_reduce_sum(p);
            l[r] = l[r] * corr + psum;
            o0[r] *= corr; o1[r] *= corr;
            m[r] = mn;
            p_lds[((int64_t)wid * QT + r) * PROW + j] = p;
        }
        // wave-local p_lds: no cross-wave use, lgkm ordering within wave is
        // guaranteed by the address dependence; no barrier needed.

        // ---- PV: lane accumulates dims (2*lane, 2*lane+1) ----
        for (int jj = 0; jj < n_here; jj++) {
            const bf162 v2 = *reinterpret_cast<const bf162*>(
                v_tile + jj * KROW + 2 * lane);
            const float v0 = bf2f(v2.x), v1 = bf2f(v2.y);
            for (int r = 0; r < rows; r++) {
                const float p = p_lds[((int64_t)wid * QT + r) * PROW + jj];
                o0[r] = fmaf(p, v0, o0[r]);
                o1[r] = fmaf(p, v1, o1[r]);
            }
        }
    }

    // ---- epilogue ----
    for (int r = 0; r < rows; r++) {
        const float linv = (l[r] > 0.f) ? 1.f / l[r] : 0.f;
        bf16* orow = out + ((int64_t)(q0 + r) * Hq + qh) * DHEAD;
        reinterpret_cast<bf162*>(orow)[lane] =
            __float22bfloat162_rn(make_float2(o0[r] * linv, o1[r] * linv));
    }
}

static int attn_lds_bytes(int G, int QT) {
    const int KROW = DHEAD + KPAD, PROW = CHUNK + 1;
    return 2 * CHUNK * KROW * 2          // k_tile + v_tile bf16
         + G * QT * DHEAD * 2            // q_lds bf16
         + G * QT * PROW * 4;            // p_lds f32
}

// Dynamic-LDS requests above the 64 KiB default (prefill tiles at G=8)
// need an explicit opt-in; CDNA4 hardware allows up to 160 KiB/workgroup.
static void allow_big_lds(const void* fn, int bytes) {
    static int done_16 = 0, done_1 = 0;
    int* flag = (fn == (const void*)k_paged_attn<16>) ? &done_16 : &done_1;
    if (!*flag && bytes > 64 * 1024) {
        (void)hipFuncSetAttribute(
            fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        *flag = 1;
    }
}

extern "C" int paged_attn_bf16(
    void* out, const void* q, const void* kpool, const void* vpool,
    const void* page_table, const void* tile_slot, const void* tile_q0,
    const void* tile_pos0, const void* tile_rows, int n_tiles, int qt,
    int Hq, int KVH, int page, int max_pages, float scale, int64_t q_stride,
    hipStream_t stream)
{
    const int G = Hq / KVH;
    dim3 grid(n_tiles, KVH);
    dim3 block(G * 64);
    if (qt == 1) {
        allow_big_lds((const void*)k_paged_attn<1>, attn_lds_bytes(G, 1));
        k_paged_attn<1><<<grid, block, attn_lds_bytes(G, 1), stream>>>(
            (bf16*)out, (const bf16*)q, (const bf16*)kpool,
            (const bf16*)vpool, (const int*)page_table,
            (const int*)tile_slot, (const int*)tile_q0,
            (const int*)tile_pos0, (const int*)tile_rows,
            Hq, KVH, page, max_pages, scale, q_stride);
    } else {
        allow_big_lds((const void*)k_paged_attn<16>, attn_lds_bytes(G, 16));
        k_paged_attn<16><<<grid, block, attn_lds_bytes(G, 16), stream>>>(
            (bf16*)out, (const bf16*)q, (const bf16*)kpool,
            (const bf16*)vpool, (const int*)page_table,
            (const int*)tile_slot, (const int*)tile_q0,
            (const int*)tile_pos0, (const int*)tile_rows,
            Hq, KVH, page, max_pages, scale, q_stride);
    }
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// SwiGLU: [T, 2F] -> [T, F], silu(gate)*up, bf16 x8 vectorized, fp32 math.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_swiglu(
    bf16* __restrict__ out, const bf16* __restrict__ gu, int T, int F)
{
    const int64_t total = (int64_t)T * F / 8;
    for (int64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = i / (F / 8), col8 = i % (F / 8);
        const bf16* g = gu + row * 2 * F + col8 * 8;
        const bf16* u = g + F;
        float vg[8], vu[8];
        load8f(g, vg);
        load8f(u, vu);
        #pragma unroll
        for (int e = 0; e < 8; e++) {
            const float sig = 1.f / (1.f + __expf(-vg[e]));
            vg[e] = vg[e] * sig * vu[e];
        }
        store8bf(out + row * F + col8 * 8, vg);
    }
}

extern "C" int swiglu_bf16(void* out, const void* gu, int T, int F,
                            hipStream_t stream)
{
    const int64_t total = (int64_t)T * F / 8;
    const int64_t want = (total + 255) / 256;
    int blocks = (int)(want < 2048 ? (want > 0 ? want : 1) : 2048);
    k_swiglu<<<blocks, 256, 0, stream>>>((bf16*)out, (const bf16*)gu, T, F);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Greedy sampler: per-row argmax over the vocab, bf16 logits.
// One 256-thread block per row; ties resolve to the LOWEST index (matches
// torch.argmax on the reference path).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_argmax(
    int* __restrict__ out, const bf16* __restrict__ logits, int V)
{
    const int row = blockIdx.x;
    const bf16* lr = logits + (int64_t)row * V;
    float best = -3.0e38f;
    int bidx = 0;
    for (int i = threadIdx.x * 8; i < V; i += blockDim.x * 8) {
        if (i + 8 <= V) {
            float v[8];
            load8f(lr + i, v);
            #pragma unroll
            for (int e = 0; e < 8; e++)
                if (v[e] > best || (v[e] == best && i + e < bidx)) {
                    best = v[e]; bidx = i + e;
                }
        } else {
            for (int e = i; e < V; e++) {
                const float v = bf2f(lr[e]);
                if (v > best || (v == best && e < bidx)) { best = v; bidx = e; }
            }
        }
    }
    // wave reduce (value, index), lowest index wins ties
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    __shared__ float wb[4];
    __shared__ int wi[4];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { wb[wid] = best; wi[wid] = bidx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < 4; wv++)
            if (wb[wv] > best || (wb[wv] == best && wi[wv] < bidx)) {
                best = wb[wv]; bidx = wi[wv];
            }
        out[row] = bidx;
    }
}

// Split-V argmax: B blocks alone (decode B=32) light 32 of 256 CUs and
// serialize ~V/2048 load rounds each (measured 45 us at V=128256).
// Stage 1: (B, SP) blocks scan V/SP slices; stage 2: one wave per row
// combines SP partials.  Global indices keep lowest-index tie-breaking.
__global__ __launch_bounds__(256) void k_argmax_part(
    float* __restrict__ pb, int* __restrict__ pi,
    const bf16* __restrict__ logits, int V, int seg)
{
    const int row = blockIdx.x, slice = blockIdx.y;
    const int lo = slice * seg, hi = min(V, lo + seg);
    const bf16* lr = logits + (int64_t)row * V;
    float best = -3.0e38f;
    int bidx = 0;
    for (int i = lo + threadIdx.x * 8; i < hi; i += blockDim.x * 8) {
        if (i + 8 <= hi) {
            float v[8];
            load8f(lr + i, v);
            #pragma unroll
            for (int e = 0; e < 8; e++)
                if (v[e] > best || (v[e] == best && i + e < bidx)) {
                    best = v[e]; bidx = i + e;
                }
        } else {
            for (int e = i; e < hi; e++) {
                const float v = bf2f(lr[e]);
                if (v > best || (v == best && e < bidx)) { best = v; bidx = e; }
            }
        }
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    __shared__ float wb[4];
    __shared__ int wi[4];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { wb[wid] = best; wi[wid] = bidx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < 4; wv++)
            if (wb[wv] > best || (wb[wv] == best && wi[wv] < bidx)) {
                best = wb[wv]; bidx = wi[wv];
            }
        pb[(int64_t)row * gridDim.y + slice] = best;
        pi[(int64_t)row * gridDim.y + slice] = bidx;
    }
}

__global__ __launch_bounds__(256) void k_argmax_comb(
    int* __restrict__ out, const float* __restrict__ pb,
    const int* __restrict__ pi, int B, int SP)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= B) return;
    float best = lane < SP ? pb[(int64_t)row * SP + lane] : -3.0e38f;
    int bidx = lane < SP ? pi[(int64_t)row * SP + lane] : 0x7fffffff;
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if (lane == 0) out[row] = bidx;
}

extern "C" int argmax_bf16(void* out, const void* logits, int B, int V,
                            void* pb, void* pi, int SP, hipStream_t stream)
{
    if (SP > 1 && pb != nullptr) {
        // 256-thread x8 rounds; ceil(V / SP): the floor gave seg = 0 for
        // V < SP and left the last V % SP tokens unscanned when V / SP
        // fell just above a multiple of 2048
        int seg = ((V + SP - 1) / SP + 2047) & ~2047;
        while ((int64_t)(SP - 1) * seg >= V) SP--;  // drop empty slices
        dim3 grid(B, SP);
        k_argmax_part<<<grid, 256, 0, stream>>>(
            (float*)pb, (int*)pi, (const bf16*)logits, V, seg);
        k_argmax_comb<<<(B + 3) / 4, 256, 0, stream>>>(
            (int*)out, (const float*)pb, (const int*)pi, B, SP);
    } else {
        k_argmax<<<B, 256, 0, stream>>>((int*)out, (const bf16*)logits, V);
    }
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------
// Fused RoPE + paged-KV append: one pass over the fresh q/k/v heads.
// q heads: rotate in place.  k heads: rotate, then write BOTH the rotated
// value in place and into the pool (k read once instead of twice).
// v heads: copy to the pool.  One launch replaces rope_bf16 + kv_append.
__global__ __launch_bounds__(256) void k_rope_append(
    bf16* __restrict__ q, bf16* __restrict__ k, const bf16* __restrict__ v,
    bf16* __restrict__ kp, bf16* __restrict__ vp,
    const int* __restrict__ pos, const int* __restrict__ slot,
    const int* __restrict__ page_table,
    const float* __restrict__ cost, const float* __restrict__ sint,
    int T, int Hq, int KVH, int D, int page, int max_pages,
    int64_t qs, int64_t ks, int64_t vs)
{
    const int gid = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int Htot = Hq + 2 * KVH;
    if (gid >= T * Htot) return;
    const int t = gid / Htot, h = gid % Htot;
    const int d2 = D / 2;
    const int p = pos[t];

    if (h < Hq) {                        // q head: rope in place
        bf16* base = q + (int64_t)t * qs + (int64_t)h * D;
        const float c = cost[(int64_t)p * d2 + lane];
        const float s = sint[(int64_t)p * d2 + lane];
        const float x1 = bf2f(base[lane]);
        const float x2 = bf2f(base[lane + d2]);
        base[lane] = f2bf(x1 * c - x2 * s);
        base[lane + d2] = f2bf(x2 * c + x1 * s);
        return;
    }
    const bool is_k = h < Hq + KVH;
    // pool row of this token for kv-head (h - Hq) or (h - Hq - KVH)
    const int64_t row = paged_kv_row(page_table, slot[t], max_pages, p, page,
                                     KVH, is_k ? h - Hq : h - Hq - KVH);
    if (is_k) {                          // k head: rope + pool write
        const int kh = h - Hq;
        bf16* base = k + (int64_t)t * ks + (int64_t)kh * D;
        bf16* dst = kp + row;
        const float c = cost[(int64_t)p * d2 + lane];
        const float s = sint[(int64_t)p * d2 + lane];
        const float x1 = bf2f(base[lane]);
        const float x2 = bf2f(base[lane + d2]);
        const bf16 lo = f2bf(x1 * c - x2 * s);
        const bf16 hi = f2bf(x2 * c + x1 * s);
        base[lane] = lo;
        base[lane + d2] = hi;
        dst[lane] = lo;
        dst[lane + d2] = hi;
        return;
    }
    {                                    // v head: pool copy
        const int vh = h - Hq - KVH;
        const bf162* src = reinterpret_cast<const bf162*>(
            v + (int64_t)t * vs + (int64_t)vh * D);
        bf162* dst = reinterpret_cast<bf162*>(vp + row);
        dst[lane] = src[lane];
    }
}

extern "C" int rope_append_bf16(
    void* q, void* k, const void* v, void* kp, void* vp, const void* pos,
    const void* slot, const void* page_table, const void* cost,
    const void* sint, int T, int Hq, int KVH, int D, int page,
    int max_pages, int64_t qs, int64_t ks, int64_t vs, hipStream_t stream)
{
    const int waves = T * (Hq + 2 * KVH);
    k_rope_append<<<(waves + 3) / 4, 256, 0, stream>>>(
        (bf16*)q, (bf16*)k, (const bf16*)v, (bf16*)kp, (bf16*)vp,
        (const int*)pos, (const int*)slot, (const int*)page_table,
        (const float*)cost, (const float*)sint,
        T, Hq, KVH, D, page, max_pages, qs, ks, vs);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Embedding gather: out[t] = table[tokens[t]]  (bf16 -> bf16, no casts).
// The torch path (index_select on a .long() cast) cost two kernels and 5%
// of the decode trace (profiles/r01_final_kernel_stats.md); this is one
// memory-bound pass of 16 B vector copies with the row indirection read
// through L1 (tokens[] is tiny).  Grid-stride so prefill T=2048 fills the
// chip and decode T=32 stays a single small launch.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_embed_gather(
    uint4* __restrict__ out, const uint4* __restrict__ table,
    const int* __restrict__ tokens, int64_t chunks_per_row, int64_t total)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; g < total; g += stride) {
        const int64_t row = g / chunks_per_row;
        const int64_t col = g - row * chunks_per_row;
        out[g] = table[(int64_t)tokens[row] * chunks_per_row + col];
    }
}

extern "C" int embed_gather_bf16(void* out, const void* table,
                                 const void* tokens, int T, int H,
                                 hipStream_t stream)
{
    const int64_t cpr = H / 8;           // 16 B chunks per row (H % 8 == 0)
    const int64_t total = (int64_t)T * cpr;
    if (total == 0) return 0;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;    // grid-stride covers the rest
    k_embed_gather<<<(int)blocks, 256, 0, stream>>>(
        (uint4*)out, (const uint4*)table, (const int*)tokens, cpr, total);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Row sum-of-squares: sq[m] = sum_k x[m][k]^2 (fp32).  Seeds the fused
// rmsnorm-in-GEMM decode chain after the embedding gather (wstream_gemm
// epilogues produce the per-tile partials for every later layer).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_row_sumsq(
    const bf16* __restrict__ x, float* __restrict__ sq, int H)
{
    const int m = blockIdx.x;
    const bf16* row = x + (int64_t)m * H;
    float s = 0.f;
    for (int i = threadIdx.x * 8; i < H; i += 256 * 8) {
        float v[8];
        load8f(row + i, v);
        #pragma unroll
        for (int j = 0; j < 8; j++) s += v[j] * v[j];
    }
    __shared__ float red[4];
    s = wave_reduce_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        sq[m] = red[0] + red[1] + red[2] + red[3];
}

extern "C" int row_sumsq_bf16(void* sq, const void* x, int M, int H,
                              hipStream_t stream)
{
    k_row_sumsq<<<M, 256, 0, stream>>>((const bf16*)x, (float*)sq, H);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Stochastic sampler: exact temperature sampling via the Gumbel-max
// trick — sampling token v with prob softmax(l/T)[v] is EXACTLY
// argmax_v(l[v]/T + g_v) with iid Gumbel noise g = -log(-log(u)).  The
// noise is counter-based (splitmix64 of (seed[row], ctr[row], v)), so a
// hipGraph replay draws fresh randomness with no host RNG round-trip
// and a request with a fixed seed reproduces its tokens regardless of
// batch composition (ctr = the sequence's own length that step).
// Rows with temps[row] <= 0 take the pure argmax path (greedy), so ONE
// captured graph serves mixed greedy/sampled batches.
// Split-V two-stage exactly like argmax (the noise is recomputed from
// (row, v) so partials stay exact).  noise_override (tests): u = that
// buffer instead of the hash.
// ---------------------------------------------------------------------------
// u = (top 23 bits + 0.5) * 2^-23: 2m + 1 < 2^24, so the sum and the
// scaling are exact in fp32 and u spans [2^-24, 1 - 2^-24].  (24 bits + 0.5
// is a rounding tie above 2^23 and reaches u == 1, i.e. g = +inf, which
// wins the argmax whatever its logit.)  The Gumbel noise is therefore
// finite, within [-2.82, 16.64], for every (seed, ctr, v).
DEV float u01_hash(uint64_t key) {
    key ^= key >> 33; key *= 0xff51afd7ed558ccdULL;
    key ^= key >> 33; key *= 0xc4ceb9fe1a85ec53ULL;
    key ^= key >> 33;
    return ((float)(key >> 41) + 0.5f) * (1.0f / 8388608.0f);
}

DEV float gumbel_of(uint64_t seed, uint64_t ctr, int v,
                    const float* noise, int64_t noff) {
    const float u = noise ? noise[noff + v]
                          : u01_hash((seed * 0x9E3779B97F4A7C15ULL)
                                     ^ (ctr * 0xD1B54A32D192ED03ULL)
                                     ^ (uint64_t)v);
    return -__logf(-__logf(u));
}

template <bool PART>
__global__ __launch_bounds__(256) void k_gumbel_part(
    int* __restrict__ out, float* __restrict__ pb, int* __restrict__ pi,
    const bf16* __restrict__ logits, const float* __restrict__ temps,
    const unsigned long long* __restrict__ seeds,
    const int* __restrict__ ctrs, const float* __restrict__ noise,
    int V, int seg)
{
    const int row = blockIdx.x, slice = PART ? blockIdx.y : 0;
    const int lo = slice * seg, hi = min(V, lo + seg);
    const bf16* lr = logits + (int64_t)row * V;
    const float T = temps ? temps[row] : 0.f;
    const bool greedy = T <= 0.f;
    const float invT = greedy ? 1.f : 1.f / T;
    const uint64_t sd = seeds ? seeds[row] : 1234567ULL;
    const uint64_t ct = ctrs ? (uint64_t)(unsigned)ctrs[row] : 0ULL;
    const int64_t noff = (int64_t)row * V;
    float best = -3.0e38f;
    int bidx = 0;
    for (int i = lo + threadIdx.x * 8; i < hi; i += blockDim.x * 8) {
        const int n = min(8, hi - i);
        float v[8];
        if (n == 8) load8f(lr + i, v);
        else for (int e = 0; e < n; e++) v[e] = bf2f(lr[i + e]);
        for (int e = 0; e < n; e++) {
            float s = v[e] * invT;
            if (!greedy)
                s += gumbel_of(sd, ct, i + e, noise, noff);
            if (s > best || (s == best && i + e < bidx)) {
                best = s; bidx = i + e;
            }
        }
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    __shared__ float wb[4];
    __shared__ int wi[4];
    const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { wb[wid] = best; wi[wid] = bidx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int wv = 1; wv < 4; wv++)
            if (wb[wv] > best || (wb[wv] == best && wi[wv] < bidx)) {
                best = wb[wv]; bidx = wi[wv];
            }
        if (PART) {
            pb[row * gridDim.y + slice] = best;
            pi[row * gridDim.y + slice] = bidx;
        } else {
            out[row] = bidx;
        }
    }
}

__global__ __launch_bounds__(64) void k_gumbel_comb(
    int* __restrict__ out, const float* __restrict__ pb,
    const int* __restrict__ pi, int sp)
{
    const int row = blockIdx.x;
    float best = -3.0e38f;
    int bidx = 0;
    for (int s = threadIdx.x; s < sp; s += 64) {
        const float v = pb[row * sp + s];
        const int ix = pi[row * sp + s];
        if (v > best || (v == best && ix < bidx)) { best = v; bidx = ix; }
    }
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if (threadIdx.x == 0) out[row] = bidx;
}

extern "C" int sample_gumbel_bf16(
    void* out, const void* logits, const void* temps, const void* seeds,
    const void* ctrs, const void* noise, int B, int V,
    void* pb, void* pi, int sp, hipStream_t stream)
{
    if (sp > 1) {
        const int seg = (V + sp - 1) / sp;
        dim3 grid(B, sp);
        k_gumbel_part<true><<<grid, 256, 0, stream>>>(
            nullptr, (float*)pb, (int*)pi, (const bf16*)logits,
            (const float*)temps, (const unsigned long long*)seeds,
            (const int*)ctrs, (const float*)noise, V, seg);
        k_gumbel_comb<<<B, 64, 0, stream>>>(
            (int*)out, (const float*)pb, (const int*)pi, sp);
    } else {
        k_gumbel_part<false><<<B, 256, 0, stream>>>(
            (int*)out, nullptr, nullptr, (const bf16*)logits,
            (const float*)temps, (const unsigned long long*)seeds,
            (const int*)ctrs, (const float*)noise, V, V);
    }
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Fragify + row sum-of-squares: convert a standard [M, H] activation into
// the 32-row MFMA fragment layout the fused decode chain streams
// (common.cuh frag_off) AND emit sq[m] = sum(x[m]^2) — one read of
// the embedding output seeds the whole chain.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fragify_sumsq(
    const bf16* __restrict__ x, bf16* __restrict__ xf,
    float* __restrict__ sq, int H)
{
    const int m = blockIdx.x;
    const bf16* row = x + (int64_t)m * H;
    // rows 32-63 land in the second 32-row frag half (MT2 chain)
    bf16* xfh = xf + (int64_t)(m >> 5) * 32 * H;
    const int mr = m & 31;
    float s = 0.f;
    for (int c = threadIdx.x; c < H / 8; c += 256) {   // 16-byte chunks
        const uint4 v = *reinterpret_cast<const uint4*>(row + c * 8);
        float f[8];
        load8f(row + c * 8, f);
        #pragma unroll
        for (int e = 0; e < 8; e++) s += f[e] * f[e];
        *reinterpret_cast<uint4*>(xfh + frag_unit(mr, c) * 8) = v;
    }
    __shared__ float red[4];
    s = wave_reduce_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        sq[m] = red[0] + red[1] + red[2] + red[3];
}

extern "C" int fragify_sumsq_bf16(void* xf, void* sq, const void* x,
                                  int M, int H, hipStream_t stream)
{
    k_fragify_sumsq<<<M, 256, 0, stream>>>(
        (const bf16*)x, (bf16*)xf, (float*)sq, H);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// Logit penalties (repeat / presence / frequency; llama.cpp order) with the
// token history kept on the device, so a penalised decode step stays inside
// the self-advancing hipGraph.  One 256-thread block per row.
//   L = clamp(lens[b], 0, max_ctx): the KV length AFTER this step's append.
//   tok[b] >= 0: hist[slot[b]][L-1] = tok[b]  (inactive rows too).
//   active row (n != 0 and not rp == 1, pp == 0, fp == 0): for every token v
//   in the window [L - min(n, L), L) with count c_v:
//       x = (x <= 0) ? x * rp : x / rp;  x -= c_v * fp + pp;  one bf16 round.
// The window's last token comes from tok[b], never read back from hist, so
// the append and the window read do not race.  Phase 1 counts with
// atomicAdd; the __threadfence() before the block barrier is what makes
// the adds complete at the barrier.  Phase 2 exchanges each
// window token's counter with 0: the one thread that receives c > 0 owns
// the token, every other occurrence receives 0.  Integer counts make the
// result independent of the order of arrival, and counts[] leaves as it
// came, all zero.  Ids outside [0, V) are skipped, never indexed with.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_logit_penalty(
    bf16* __restrict__ logits, int* __restrict__ hist,
    const int* __restrict__ slot, const int* __restrict__ lens,
    const int* __restrict__ tok, const int* __restrict__ last_n,
    const float* __restrict__ rp, const float* __restrict__ pp,
    const float* __restrict__ fp, int* __restrict__ counts,
    int V, int max_ctx, int max_slots)
{
    const int b = blockIdx.x;
    const int sl = slot[b];
    if (sl < 0 || sl >= max_slots) return;
    const int L = min(max(lens[b], 0), max_ctx);
    const int t_in = tok[b];
    int* hrow = hist + (int64_t)sl * max_ctx;
    if (threadIdx.x == 0 && t_in >= 0 && L >= 1) hrow[L - 1] = t_in;
    const int n = last_n[b];
    const float r = rp[b], p = pp[b], f = fp[b];
    if (n == 0 || (r == 1.f && p == 0.f && f == 0.f)) return;
    const int w = (n < 0 || n > L) ? L : n;
    const int lo = L - w;
    bf16* lrow = logits + (int64_t)b * V;
    int* crow = counts + (int64_t)b * V;
    // both loops walk the same window positions per thread
    for (int i = lo + threadIdx.x; i < L; i += 256) {
        const int t = (i == L - 1 && t_in >= 0) ? t_in : hrow[i];
        if (t >= 0 && t < V) (void)atomicAdd(&crow[t], 1);
    }
    __threadfence();
    __syncthreads();
    for (int i = lo + threadIdx.x; i < L; i += 256) {
        const int t = (i == L - 1 && t_in >= 0) ? t_in : hrow[i];
        if (t < 0 || t >= V) continue;
        const int c = atomicExch(&crow[t], 0);
        if (c > 0) {
            float x = bf2f(lrow[t]);
            // each step rounded on its own (no fma contraction), so the
            // fp32 host reference computes the same bits
            x = (x <= 0.f) ? __fmul_rn(x, r) : __fdiv_rn(x, r);
            x = __fsub_rn(x, __fadd_rn(__fmul_rn((float)c, f), p));
            lrow[t] = f2bf(x);
        }
    }
}

extern "C" int logit_penalty_bf16(
    void* logits, void* hist, const void* slot, const void* lens,
    const void* tok, const void* last_n, const void* rp, const void* pp,
    const void* fp, void* counts, int B, int V, int max_ctx, int max_slots,
    hipStream_t stream)
{
    if (B == 0) return 0;
    k_logit_penalty<<<B, 256, 0, stream>>>(
        (bf16*)logits, (int*)hist, (const int*)slot, (const int*)lens,
        (const int*)tok, (const int*)last_n, (const float*)rp,
        (const float*)pp, (const float*)fp, (int*)counts, V, max_ctx,
        max_slots);
    return (int)hipGetLastError();
}
