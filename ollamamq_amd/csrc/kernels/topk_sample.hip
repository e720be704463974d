// Top-k / top-p sampling of bf16 logits in two launches, nothing allocated,
// nothing zeroed, no global atomics (contract: docs/KERNELS.md, "Top-k/top-p
// sampling kernel"; host wrapper: ops/hip.py sample_topk).
//
// A bf16 logit's order is fully determined by a 16-bit key, so the exact
// C = min(256, V) largest of a row are a two-level 256-bin radix select:
//
//   k_topk_part  grid (B, SP): one pass over a V/SP slice.  LDS histogram of
//                the key's high byte, written per slice with plain stores,
//                and the slice's (max, sum exp((l - max) / T)) partial.
//   k_topk_pick  one 1024-thread block per row.  Sums the slice histograms
//                and finds the high byte b1 of the C-th largest key; a second
//                pass over the row histograms the low byte of the keys in
//                bin b1, which gives the threshold key tau exactly; a third
//                pass collects every key > tau and the lowest-id keys == tau;
//                the C entries are ranked in LDS on (key, ~id); then one
//                thread per rank applies top-k / top-p on the full-vocabulary
//                probabilities and takes the Gumbel-max among the kept ranks.
#include "common.cuh"

#define TOPC 256                  // candidates per row
#define PICK_T 1024               // threads of k_topk_pick
#define PICK_W (PICK_T / 64)

// bf16 bits -> 16-bit key whose unsigned order is the value order; -0.0 and
// +0.0 share a key, -inf is the lowest key of a non-NaN value.
DEV unsigned key16(unsigned bits) {
    bits &= 0xffffu;
    if ((bits & 0x7fffu) == 0) bits = 0;
    return bits ^ ((bits & 0x8000u) ? 0xffffu : 0x8000u);
}

DEV float key_value(unsigned key) {
    const unsigned bits = key ^ ((key & 0x8000u) ? 0x8000u : 0xffffu);
    return __uint_as_float(bits << 16);
}

DEV float bits_value(unsigned bits) { return __uint_as_float(bits << 16); }

// The 8 bf16 at elements c .. c+7 of row p, restricted to [lo, hi); returns
// the mask of the elements read.  c is congruent to -mis modulo 8, where mis
// is the row's offset in elements from a 16-byte boundary, so the full group
// is one aligned 16-byte load whatever V % 8 is.
DEV unsigned load8bits(const unsigned short* p, int c, int lo, int hi,
                       unsigned* bits) {
    if (c >= lo && c + 8 <= hi) {
        const uint4 q = *reinterpret_cast<const uint4*>(p + c);
        bits[0] = q.x & 0xffffu; bits[1] = q.x >> 16;
        bits[2] = q.y & 0xffffu; bits[3] = q.y >> 16;
        bits[4] = q.z & 0xffffu; bits[5] = q.z >> 16;
        bits[6] = q.w & 0xffffu; bits[7] = q.w >> 16;
        return 0xffu;
    }
    unsigned m = 0;
    #pragma unroll
    for (int e = 0; e < 8; e++) {
        const int i = c + e;
        bits[e] = 0;
        if (i >= lo && i < hi) { bits[e] = p[i]; m |= 1u << e; }
    }
    return m;
}

DEV int row_misalign(const unsigned short* p) {
    return (int)((reinterpret_cast<uintptr_t>(p) >> 1) & 7);
}

// f(id, bits) for every element of [lo, hi), nthr threads interleaved
template <class F>
DEV void for_each_elem(const unsigned short* p, int lo, int hi, int tid,
                       int nthr, F f) {
    const int mis = row_misalign(p);
    for (int c = ((lo + mis) & ~7) - mis + tid * 8; c < hi; c += nthr * 8) {
        unsigned bits[8];
        const unsigned m = load8bits(p, c, lo, hi, bits);
        #pragma unroll
        for (int e = 0; e < 8; e++)
            if ((m >> e) & 1) f(c + e, bits[e]);
    }
}

// ---------------------------------------------------------------------------
// Stage 1
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_topk_part(
    unsigned* __restrict__ hist1, float* __restrict__ part,
    const bf16* __restrict__ logits, const float* __restrict__ temps,
    int V, int seg)
{
    const int row = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int lo = slice * seg, hi = min(V, lo + seg);
    const unsigned short* lr = reinterpret_cast<const unsigned short*>(
        logits + (int64_t)row * V);
    const int64_t cell = (int64_t)row * gridDim.y + slice;
    __shared__ unsigned hist[256];
    __shared__ unsigned wmax[4];
    __shared__ float wsum[4];

    hist[tid] = 0;
    __syncthreads();
    unsigned kmax = 0;
    for_each_elem(lr, lo, hi, tid, 256, [&](int, unsigned bits) {
        const unsigned k = key16(bits);
        atomicAdd(&hist[k >> 8], 1u);
        kmax = max(kmax, k);
    });
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off, 64));
    if (lane == 0) wmax[wid] = kmax;
    __syncthreads();
    hist1[cell * 256 + tid] = hist[tid];

    const float T = temps[row];
    if (T <= 0.f) return;               // greedy row: no probabilities
    kmax = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    const float m = key_value(kmax);
    float s = 0.f;
    if (m > -INFINITY)                  // a slice of -inf only adds no mass
        for_each_elem(lr, lo, hi, tid, 256, [&](int, unsigned bits) {
            s += expf(__fdiv_rn(bits_value(bits) - m, T));
        });
    s = wave_reduce_sum(s);
    if (lane == 0) wsum[wid] = s;
    __syncthreads();
    if (tid == 0) {
        part[cell * 2] = m;
        part[cell * 2 + 1] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    }
}

// ---------------------------------------------------------------------------
// Stage 2
// ---------------------------------------------------------------------------
// Wave 0: the highest bin whose suffix count (itself and every bin above)
// reaches `want` (>= 1), and the count of the bins above it (< want).  Lane l
// owns bins 4l .. 4l+3.  sel = {bin, count above}.
DEV void pick_bin(const unsigned* hist, unsigned want, int* sel, int lane) {
    const uint4 q = *reinterpret_cast<const uint4*>(hist + lane * 4);
    const unsigned h[4] = {q.x, q.y, q.z, q.w};
    const unsigned t = h[0] + h[1] + h[2] + h[3];
    unsigned suf = t;                   // lanes >= this one
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned o = (unsigned)__shfl_down((int)suf, off, 64);
        if (lane + off < 64) suf += o;
    }
    if (lane == 0) { sel[0] = 0; sel[1] = 0; }
    unsigned run = suf - t;             // keys in the bins above this lane's
    #pragma unroll
    for (int e = 3; e >= 0; e--) {
        if (run < want && run + h[e] >= want) {
            sel[0] = lane * 4 + e;
            sel[1] = (int)run;
        }
        run += h[e];
    }
}

DEV unsigned long long entry_of(unsigned key, int id) {
    return ((unsigned long long)key << 32) | (unsigned)~id;
}

__global__ __launch_bounds__(PICK_T) void k_topk_pick(
    int* __restrict__ out, float* __restrict__ cvals, int* __restrict__ cids,
    int* __restrict__ cpick, const unsigned* __restrict__ hist1,
    const float* __restrict__ part, const bf16* __restrict__ logits,
    const float* __restrict__ temps, const long long* __restrict__ top_k,
    const float* __restrict__ top_p,
    const unsigned long long* __restrict__ seeds,
    const int* __restrict__ ctrs, int V, int SP)
{
    const int row = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int C = min(TOPC, V);
    const unsigned short* lr = reinterpret_cast<const unsigned short*>(
        logits + (int64_t)row * V);
    __shared__ __align__(16) unsigned hist[256];
    __shared__ unsigned long long ent[TOPC], srt[TOPC];
    __shared__ int tie[PICK_W][TOPC];
    __shared__ int tie_n[PICK_W];
    __shared__ int sel[2];
    __shared__ unsigned n_list;
    __shared__ float wtot[4], wbest[4];
    __shared__ int widx[4];

    // ---- level 1: the slices' high-byte histograms -> b1, n_above
    if (tid < 256) {
        unsigned h = 0;
        for (int s = 0; s < SP; s++)
            h += hist1[((int64_t)row * SP + s) * 256 + tid];
        hist[tid] = h;
        ent[tid] = 0;                   // ranks >= C (V < 256) stay zero
    }
    if (tid == 0) n_list = 0;
    __syncthreads();
    if (wid == 0) pick_bin(hist, (unsigned)C, sel, lane);
    __syncthreads();
    const unsigned b1 = (unsigned)sel[0];
    const int n_above = sel[1];
    if (tid < 256) hist[tid] = 0;
    __syncthreads();

    // ---- level 2: low byte of the keys in bin b1 -> tau, n_gt, need
    for_each_elem(lr, 0, V, tid, PICK_T, [&](int, unsigned bits) {
        const unsigned k = key16(bits);
        if ((k >> 8) == b1) atomicAdd(&hist[k & 255u], 1u);
    });
    __syncthreads();
    if (wid == 0) pick_bin(hist, (unsigned)(C - n_above), sel, lane);
    __syncthreads();
    const unsigned tau = (b1 << 8) | (unsigned)sel[0];
    const int n_gt = n_above + sel[1];  // keys > tau, < C
    const int need = C - n_gt;          // keys == tau to take, >= 1

    // ---- collect.  Keys > tau go to ent[] through an LDS counter in any
    // order (the ranking fixes it).  Keys == tau must be taken lowest id
    // first: each wave walks a contiguous span of the row in ascending id,
    // numbers its ties with a wave prefix sum and keeps the first `need` of
    // them; the waves' lists are joined in wave order below.
    {
        const int mis = row_misalign(lr);
        const int span = (V + PICK_W - 1) / PICK_W;
        const int lo = min(V, wid * span), hi = min(V, lo + span);
        int wbase = 0;                  // wave-uniform: ties seen so far
        for (int c0 = ((lo + mis) & ~7) - mis; c0 < hi; c0 += 512) {
            const int c = c0 + lane * 8;
            unsigned bits[8];
            const unsigned m = c < hi ? load8bits(lr, c, lo, hi, bits) : 0u;
            unsigned eq = 0;
            #pragma unroll
            for (int e = 0; e < 8; e++) {
                if (!((m >> e) & 1)) continue;
                const unsigned k = key16(bits[e]);
                if (k > tau) {
                    const unsigned pos = atomicAdd(&n_list, 1u);
                    if (pos < TOPC) ent[pos] = entry_of(k, c + e);
                } else if (k == tau) {
                    eq |= 1u << e;
                }
            }
            const int n = __popc(eq);
            if (__ballot(n > 0) != 0ull && wbase < need) {
                int incl = n;
                #pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(incl, off, 64);
                    if (lane >= off) incl += o;
                }
                int at = wbase + incl - n;
                #pragma unroll
                for (int e = 0; e < 8; e++)
                    if ((eq >> e) & 1) {
                        if (at < need) tie[wid][at] = c + e;
                        at++;
                    }
                wbase += __shfl(incl, 63, 64);
            }
        }
        if (lane == 0) tie_n[wid] = min(wbase, need);
    }
    __syncthreads();
    {
        int base = 0;
        for (int w = 0; w < wid; w++) base += tie_n[w];
        const int n = tie_n[wid];
        for (int r = lane; r < n; r += 64)
            if (base + r < need)
                ent[n_gt + base + r] = entry_of(tau, tie[wid][r]);
    }
    __syncthreads();

    // ---- rank the 256 entries on (key, ~id), descending: value descending,
    // id ascending among equal values.  One counting pass of broadcast LDS
    // reads; the zero pads (equal among themselves) are ordered by slot.
    if (tid < TOPC) {
        const unsigned long long mine = ent[tid];
        int rank = 0;
        for (int j = 0; j < TOPC; j++) {
            const unsigned long long o = ent[j];
            rank += (o > mine || (o == mine && j < tid)) ? 1 : 0;
        }
        srt[rank] = mine;
    }
    __syncthreads();

    // ---- one thread per rank
    const int c = tid;
    const bool live = c < C;
    const unsigned long long e = live ? srt[c] : 0ull;
    const float v = live ? key_value((unsigned)(e >> 32)) : -INFINITY;
    // ids come from the row walk and lie in [0, V); the clamp only keeps a
    // zero pad from ever leaving the kernel as an id
    const int id = (int)min(~(unsigned)e, (unsigned)(V - 1));
    const float T = temps[row];
    const int64_t co = (int64_t)row * TOPC + c;
    if (T <= 0.f) {                     // greedy: rank 0, nothing filtered
        if (live && cvals) { cvals[co] = v; cids[co] = id; }
        if (tid == 0) {
            out[row] = id;
            if (cpick) cpick[row] = 0;
        }
        return;
    }
    float p = 0.f;
    if (live) {
        float M = -INFINITY, S = 0.f;
        for (int s = 0; s < SP; s++)
            M = fmaxf(M, part[((int64_t)row * SP + s) * 2]);
        for (int s = 0; s < SP; s++) {
            const float m = part[((int64_t)row * SP + s) * 2];
            if (m > -INFINITY)
                S += part[((int64_t)row * SP + s) * 2 + 1]
                     * expf(__fdiv_rn(m - M, T));
        }
        // p = exp(v/T - lse) with lse = M/T + log S, the maximum subtracted
        // before the division so that a low temperature costs no precision
        p = expf(__fdiv_rn(v - M, T) - logf(S));
    }
    float incl = p;                     // exclusive scan of p over the ranks
    #pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    const float prev = __shfl_up(incl, 1, 64);
    if (wid < 4 && lane == 63) wtot[wid] = incl;
    __syncthreads();
    float before = lane ? prev : 0.f;
    if (wid < 4) {
        float base = 0.f;
        for (int w = 0; w < wid; w++) base += wtot[w];
        before += base;
    }
    long long k = top_k[row];
    k = k < 1 ? 1 : (k > C ? C : k);
    const float tp = top_p[row];
    const bool keep = live && (c == 0 ||
        (c < k && (tp >= 1.f || before < tp) && isfinite(v)));
    const float invT = 1.f / T;
    float best = -INFINITY;
    int bidx = c;
    if (keep)
        best = v * invT + gumbel_of(seeds[row], (uint64_t)(unsigned)ctrs[row],
                                    c, nullptr, 0);
    #pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_down(best, off, 64);
        const int oi = __shfl_down(bidx, off, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if (wid < 4 && lane == 0) { wbest[wid] = best; widx[wid] = bidx; }
    if (live && cvals) { cvals[co] = keep ? v : -INFINITY; cids[co] = id; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; w++)
            if (wbest[w] > best || (wbest[w] == best && widx[w] < bidx)) {
                best = wbest[w]; bidx = widx[w];
            }
        bidx = min(max(bidx, 0), C - 1);
        out[row] = (int)min(~(unsigned)srt[bidx], (unsigned)(V - 1));
        if (cpick) cpick[row] = bidx;
    }
}

// hist1: B * SP * 256 uint32, part: B * SP * 2 fp32 (both written before
// they are read, every launch).  cvals / cids / cpick may be null together.
extern "C" int sample_topk_bf16(
    void* out, const void* logits, const void* temps, const void* top_k,
    const void* top_p, const void* seeds, const void* ctrs, int B, int V,
    void* hist1, void* part, int SP, void* cvals, void* cids, void* cpick,
    hipStream_t stream)
{
    if (B <= 0 || V <= 0 || SP <= 0) return (int)hipErrorInvalidValue;
    const int seg = (((V + SP - 1) / SP) + 7) & ~7;
    while (SP > 1 && (int64_t)(SP - 1) * seg >= V) SP--;   // no empty slice
    k_topk_part<<<dim3(B, SP), 256, 0, stream>>>(
        (unsigned*)hist1, (float*)part, (const bf16*)logits,
        (const float*)temps, V, seg);
    k_topk_pick<<<B, PICK_T, 0, stream>>>(
        (int*)out, (float*)cvals, (int*)cids, (int*)cpick,
        (const unsigned*)hist1, (const float*)part, (const bf16*)logits,
        (const float*)temps, (const long long*)top_k, (const float*)top_p,
        (const unsigned long long*)seeds, (const int*)ctrs, V, SP);
    return (int)hipGetLastError();
}
