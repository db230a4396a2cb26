// select.hip -- the quantile and scale selections of an outlier-filter chain (Trimmed / Median / VarTrimmed limits, the scale estimators of
// RobustOutlierFilter).  In: the matcher's d2 (icpmi_ctx::d_d2), the loop state and the handle's selection histograms (d_selhist); out:
// IcpState::limits[] (robust_med / robust_scale for the estimators).  The last level of the FUSED selection is resolved by its consumers
// (loop.hip: accumulate_kernel, res_pairs_kernel) with common.h's block_find_rank_2tier.  enqueue_selection puts the launches on the
// handle's stream, selection_reserve sizes what they need before a capture starts.
#include "common.h"
#include <cstring>
#include <vector>

namespace {

// ---------------------------------------------------------------------------------------------
// quantile selection == Matches::getDistsQuantile: over entries that are finite
// and > 0, element of rank (size_t)(count * quantile) [float product], quantile == 1 -> max.
// d2 >= 0 so the IEEE bit pattern orders like an unsigned integer: 3 radix passes 11/11/10 bits.
// ---------------------------------------------------------------------------------------------
// MODE 0: the quantile of the finite positive d2 (getDistsQuantile); MODE 3: the same values, at iteration 1 only
// (RobustOutlierFilter{scaleEstimator: berg}).  MODE 1 / 2: RobustOutlierFilter{scaleEstimator: mad} --
// Matches::getMedianAbsDeviation takes every finite d2 (zeros included): 1 = the values themselves, 2 = |d2 - median|;
// nb_scale: the estimate is only refreshed while iteration <= nbIterationForScale (0 = always).
template <int PASS, int MODE = 0>
__global__ __launch_bounds__(256) void sel_hist_kernel(const float* __restrict__ d2, int64_t count,
                                                       const IcpState* __restrict__ st, unsigned* __restrict__ ghist, int nb_scale = 0)
{
    if (st->done) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) nn_stamp_close(const_cast<IcpState*>(st));
    if (MODE != 0 && nb_scale != 0 && st->iter + 1 > nb_scale) return;
    if (MODE == 3 && st->iter != 0) return; // berg: the median is taken at iteration 1 only
    __shared__ unsigned h[ICPMI_SEL_BINS];
    for (int b = threadIdx.x; b < ICPMI_SEL_BINS; b += 256) h[b] = 0;
    __syncthreads();
    const unsigned prefix = st->sel_prefix;
    const float med = MODE == 2 ? st->robust_med : 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        float v = d2[i];
        if (MODE == 0 || MODE == 3) { if (!(v != INFINITY && v > 0.f)) continue; }
        else {
            if (v == INFINITY) continue;
            if (MODE == 2) v = fabsf(v - med);
        }
        const unsigned bits = __float_as_uint(v);
        if (PASS == 0) atomicAdd(&h[bits >> 21], 1u);
        else if (PASS == 1) { if ((bits >> 21) == prefix) atomicAdd(&h[(bits >> 10) & 2047u], 1u); }
        else { if ((bits >> 10) == prefix) atomicAdd(&h[bits & 1023u], 1u); }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < ICPMI_SEL_BINS; b += 256)
        if (h[b]) atomicAdd(&ghist[b], h[b]);
}

// RobustOutlierFilter{scaleEstimator: std}: Matches::getStandardDeviation over EVERY entry of the distance matrix.  Two rounds
// (PASS 0: sum d -> mean, kept in robust_med; PASS 1: sum (d - mean)^2 -> robust_scale = sqrt(sqrt(sum / (size - 1)))), each a
// fixed grid of fixed-order partial sums in double (`part`, one per workgroup) and a one-workgroup tail: same bits every run.
template <int PASS>
__global__ __launch_bounds__(256) void std_part_kernel(const float* __restrict__ d2, int64_t count, const IcpState* __restrict__ st,
                                                       double* __restrict__ part, int nb_scale)
{
    if (st->done) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) nn_stamp_close(const_cast<IcpState*>(st));
    if (nb_scale != 0 && st->iter + 1 > nb_scale) return;
    __shared__ double sh[256];
    const float mean = PASS == 1 ? st->robust_med : 0.f;
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        const float v = d2[i];
        if (PASS == 0) s += (double)v;
        else { const float dv = __fsub_rn(v, mean); s += (double)__fmul_rn(dv, dv); }
    }
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

template <int PASS>
__global__ __launch_bounds__(256) void std_tail_kernel(IcpState* __restrict__ st, const double* __restrict__ part, int nparts, int64_t count,
                                                       int nb_scale)
{
    if (st->done) return;
    if (nb_scale != 0 && st->iter + 1 > nb_scale) return;
    __shared__ double sh[256];
    sh[threadIdx.x] = (int)threadIdx.x < nparts ? part[threadIdx.x] : 0.0;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (PASS == 0) st->robust_med = (float)(sh[0] / (double)count);
        else st->robust_scale = sqrtf(sqrtf((float)sh[0] / (float)(count - 1)));
    }
}

// single workgroup: locate the bin holding the wanted rank, narrow prefix / rank, clear the histogram
template <int PASS>
__global__ __launch_bounds__(256) void sel_scan_kernel(IcpState* __restrict__ st, unsigned* __restrict__ ghist, float quantile,
                                                       int filter_slot, int is_median, float factor, int dest = 0, int nb_scale = 0)
{
    // dest 0: limits[filter_slot] (quantile filters); 1: robust_med, 2: robust_scale = sqrt(mad) -- rank size / 2 (quantile < 0);
    // 3: berg -- robust_scale = 1.9 sqrt(quantile) at iteration 1, 0.85 (scale - target) + target afterwards (factor = target)
    if (st->done) return;
    if (dest != 0 && nb_scale != 0 && st->iter + 1 > nb_scale) return;
    if (dest == 3 && st->iter != 0) {
        if (PASS == 2 && threadIdx.x == 0) st->robust_scale = __fadd_rn(__fmul_rn(0.85f, __fsub_rn(st->robust_scale, factor)), factor);
        return;
    }
    __shared__ unsigned sh[256];
    __shared__ unsigned s_rank;
    const int t = threadIdx.x;
    unsigned v[8], s = 0;
    for (int e = 0; e < 8; ++e) { v[e] = ghist[t * 8 + e]; s += v[e]; ghist[t * 8 + e] = 0; }
    sh[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned add = t >= off ? sh[t - off] : 0u;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned incl = sh[t], excl = incl - s, total = sh[255];
    if (t == 0) {
        if (PASS == 0) {
            st->n_valid = total;
            if (total == 0) { st->error = ICPMI_ERR_NO_OUTLIER_TO_FILTER; st->done = 1; s_rank = 0; }
            else {
                unsigned r;
                if (quantile < 0.f) r = total / 2;
                else if (quantile == 1.0f) r = total - 1;
                else {
                    r = (unsigned)((float)total * quantile);
                    if (r > total - 1) r = total - 1;
                }
                s_rank = r;
            }
        } else s_rank = st->sel_rank;
    }
    __syncthreads();
    if (total == 0) return;
    const unsigned rank = s_rank;
    if (rank >= excl && rank < incl) {
        unsigned acc = excl;
        int bin = t * 8;
        for (int e = 0; e < 8; ++e) {
            if (rank < acc + v[e]) { bin = t * 8 + e; break; }
            acc += v[e];
        }
        const unsigned prev = PASS == 0 ? 0u : st->sel_prefix;
        const unsigned np = PASS == 0 ? (unsigned)bin : (PASS == 1 ? ((prev << 11) | (unsigned)bin) : ((prev << 10) | (unsigned)bin));
        st->sel_prefix = np;
        st->sel_rank = rank - acc;
        if (PASS == 2) {
            const float q = __uint_as_float(np);
            if (dest == 1) st->robust_med = q;
            else if (dest == 2) st->robust_scale = sqrtf(q);
            else if (dest == 3) st->robust_scale = (float)(1.9 * (double)sqrtf(q));
            else st->limits[filter_slot] = is_median ? factor * q : q;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Fused selection (exactly one quantile-type filter in the chain -- the common case).  Two 16-bit
// radix levels (common.h: ICPMI_S2_*), chain per iteration
//   NN (builds level 0) -> sel2_scan_hist (scans level 0, builds level 1) -> [scan level 1 + pair sums] -> solve.
// Every workgroup of a consumer kernel redoes the scan of the histogram it needs (256 coarse bins,
// then the 256 fine bins under the selected coarse one: common.h, block_find_rank_2tier) -- cheaper than a kernel boundary.
// Clearing: level 0 is cleared by the pair-sum kernel (after its last reader), level 1 by whoever
// builds level 0 of the next iteration (before its next builder).
// ---------------------------------------------------------------------------------------------
// (r5) The speculative window of the k > 1 loop (common.h: ICPMI_S2_WIN; counted by nnk_wg_kernel around the previous iteration's prefix).
// All 256 threads call; true = the selected rank lies in one of the window's bins: `prefix` is that bin, `rank_rem` the rank inside it,
// `total` the number of finite positive distances -- what block_find_rank_2tier would return from a full level 0, without one.
// false = no window this iteration, or the rank falls below / above it (the caller goes on with the full histogram).
__device__ __forceinline__ bool win_lookup(const unsigned* __restrict__ hists, float quantile, unsigned* sh /* >= 16 words */,
                                           unsigned& prefix, unsigned& rank_rem, unsigned& total)
{
    const unsigned long long* __restrict__ W = reinterpret_cast<const unsigned long long*>(hists + ICPMI_S2_WIN);
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    // wave w < 3 sums word w over the copies (the packed fields cannot carry: every field's total is below 2^21), wave 3 fetches the header
    static_assert(ICPMI_WIN_COPIES <= 64, "one lane per copy");
    unsigned long long v = 0ull;
    if (w < 3) { if (l < ICPMI_WIN_COPIES) v = W[(size_t)(l * 3 + w) * ICPMI_WIN_PAD]; }
    else if (l == 0) v = W[ICPMI_WIN_HDR];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
    if (l == 0) {
        if (w < 3) {
#pragma unroll
            for (int j = 0; j < 3; ++j) sh[3 * w + j] = (unsigned)(v >> (21 * j)) & 0x1fffffu;
        } else sh[9] = (unsigned)v;
    }
    __syncthreads();
    if (t == 0) {
        const unsigned lo1 = sh[9], below = sh[0], above = sh[ICPMI_WIN_BINS + 1];
        unsigned inwin = 0u;
        for (int b = 0; b < ICPMI_WIN_BINS; ++b) inwin += sh[1 + b];
        const unsigned tot = below + inwin + above;
        unsigned hit = 0u, pf = 0u, rr = 0u;
        if (lo1 != 0u && tot != 0u) {
            unsigned rank; // getDistsQuantile's index, as block_find_rank256 forms it
            if (quantile == 1.0f) rank = tot - 1;
            else {
                rank = (unsigned)((float)tot * quantile);
                if (rank > tot - 1) rank = tot - 1;
            }
            if (rank >= below && rank - below < inwin) {
                unsigned r = rank - below;
                for (int b = 0; b < ICPMI_WIN_BINS; ++b) {
                    const unsigned cb = sh[1 + b];
                    if (r < cb) { pf = lo1 - 1u + (unsigned)b; rr = r; hit = 1u; break; }
                    r -= cb;
                }
            }
        }
        sh[10] = hit; sh[11] = pf; sh[12] = rr; sh[13] = tot;
    }
    __syncthreads();
    const bool hit = sh[10] != 0u;
    prefix = sh[11]; rank_rem = sh[12]; total = sh[13];
    __syncthreads();
    return hit;
}

// level-0 histograms as a stand-alone kernel (NN variants that do not build them: k > 1, chains that may
// need the brute-force pass).  Also clears level 1, like the NN kernel does when it is the builder.
__global__ __launch_bounds__(256) void sel2_hist0_kernel(const float* __restrict__ d2, BatchArgs ba, int k, const IcpState* __restrict__ st,
                                                         unsigned* __restrict__ hists, float quantile, int use_win)
{
    const int64_t count = (int64_t)ba.n[blockIdx.y] * k; // blockIdx.y = reading of a batch
    d2 += (size_t)blockIdx.y * (size_t)ba.qstride * k;
    hists += (size_t)blockIdx.y * ICPMI_SELHIST_WORDS;
    st += blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0 && !st->done) nn_stamp_close(const_cast<IcpState*>(st));
    if (use_win) { // (r5) the NN kernel's window holds the selected element (and that kernel cleared level 1): nothing to do in this launch
        if (st->done) return;
        __shared__ unsigned shw[16];
        unsigned pf, rr, tot;
        if (win_lookup(hists, quantile, shw, pf, rr, tot)) return;
    }
#ifndef ICPMI_H0_PF
#define ICPMI_H0_PF 16
#endif
    constexpr int PF = ICPMI_H0_PF; // all of a thread's matches in flight before the first LDS atomic (4096 per workgroup: 16 per thread)
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float pv[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) pv[u] = i0 + u * stride < count ? d2[i0 + u * stride] : INFINITY;
    if (st->done) return;
    // Fine bins (top 16 bits of d^2) are counted in LDS first, in a direct-mapped window of 4096 bins = 32 octaves that ends
    // just above the largest value of the workgroup's FIRST batch of matches (the matches of a launch span a few octaves below
    // the matcher's radius; whatever falls outside goes to memory directly): ONE LDS atomic per match -- r2 used a 1024-slot hash
    // (compare-and-swap, then the count) plus the coarse bin, three dependent LDS atomics on addresses that most lanes of a
    // wave share.  The coarse bins are summed from the window when it is flushed.
    constexpr int WIN = 4096;
    __shared__ unsigned h[256];
    __shared__ unsigned win[WIN];
    __shared__ unsigned s_top;
    h[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < WIN; i += 256) win[i] = 0;
    if (threadIdx.x == 0) s_top = 0u;
#if ICPMI_WT_CLEAR
    clear_words_wt(hists + ICPMI_S2_C1, 256 + 65536, i0, stride);
#else
    for (int64_t i = i0; i < 256 + 65536; i += stride) hists[ICPMI_S2_C1 + i] = 0;
#endif
    __syncthreads();
    {
        unsigned mx = 0;
#pragma unroll
        for (int u = 0; u < PF; ++u) if (pv[u] != INFINITY && pv[u] > 0.f) mx = max(mx, __float_as_uint(pv[u]) >> 16);
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
        if ((threadIdx.x & 63) == 0 && mx) atomicMax(&s_top, mx);
    }
    __syncthreads();
    const unsigned top = s_top + 1u, lo = top > (unsigned)WIN ? top - (unsigned)WIN : 0u;
    unsigned* fine = hists + ICPMI_S2_F0 + (blockIdx.x % ICPMI_S2_FCOPIES) * 65536;
    auto add = [&](float v) {
        if (!(v != INFINITY && v > 0.f)) return;
        const unsigned bits = __float_as_uint(v);
        const unsigned bin = bits >> 16, rel = bin - lo;
        if (rel < (unsigned)WIN) atomicAdd(&win[rel], 1u);
        else { atomicAdd(&h[bits >> 24], 1u); atomicAdd(&fine[ICPMI_S2_FIDX(bin)], 1u); }
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) add(pv[u]);
    for (int64_t i = i0 + PF * stride; i < count; i += stride) add(d2[i]);
    __syncthreads();
    for (int i = threadIdx.x; i < WIN; i += 256) {
        const unsigned cnt = win[i];
        if (cnt) { const unsigned bin = lo + (unsigned)i; atomicAdd(&h[bin >> 8], cnt); atomicAdd(&fine[ICPMI_S2_FIDX(bin)], cnt); }
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hists[ICPMI_S2_C0 + (blockIdx.x % ICPMI_S2_COPIES) * 256 + threadIdx.x], h[threadIdx.x]);
}

// scan level 0 (top 16 bits), build level 1 (low 16 bits) from the elements under the selected prefix
__global__ __launch_bounds__(256) void sel2_scan_hist_kernel(const float* __restrict__ d2, BatchArgs ba, int k, IcpState* __restrict__ st,
                                                             unsigned* __restrict__ hists, float quantile, int use_win)
{
    // blockIdx.y = reading of a batch (common.h: BatchArgs)
    asm volatile("" ::"s"(ba.n[blockIdx.y]), "s"(ba.qstride), "s"(k), "s"(d2), "s"(hists), "s"(st), "s"(quantile), "s"(use_win)); // the kernel arguments in one batch (as in nn.hip)
    const int64_t count = (int64_t)ba.n[blockIdx.y] * k;
    d2 += (size_t)blockIdx.y * (size_t)ba.qstride * k;
    hists += (size_t)blockIdx.y * ICPMI_SELHIST_WORDS;
    st += blockIdx.y;
    // first trip: the loop header, the lane's elements and the coarse counts are requested together and joined below -- nothing of the
    // loop state is read from memory after that
    constexpr int PF = 2;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    HdrView hv{hdr_load(st)};
    float pv[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) pv[u] = i0 + u * stride < count ? d2[i0 + u * stride] : INFINITY;
    unsigned cv = 0;
#pragma unroll
    for (int cpy = 0; cpy < ICPMI_S2_COPIES; ++cpy) cv += hists[ICPMI_S2_C0 + cpy * 256 + threadIdx.x];
    asm volatile("" : "+v"(hv.w), "+v"(pv[0]), "+v"(pv[1]), "+v"(cv)); // the join
    if (hv.i(ICPMI_HDR_W(done))) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) nn_stamp_close(st, hv.u64(ICPMI_HDR_W(t_nn_begin)));
    __shared__ unsigned sh[16];
    unsigned prefix, rem, total;
    // (r5) k > 1: the NN kernel's window around the previous prefix first (the stand-alone builder took the same decision from the same words)
    const bool win_hit = use_win && win_lookup(hists, quantile, sh, prefix, rem, total);
    // (the shuffle scan: with common.h's register scan this kernel traced 5.24 against 5.36 us, inside the 0.24 us its own runs differ by --
    // DESIGN.md 4.2, profiles/tail_dpp_kernel_stats.csv)
    if (!win_hit) block_find_rank_2tier<ICPMI_S2_FCOPIES, false>(cv, hists + ICPMI_S2_F0, true, quantile, 0u, sh, prefix, rem, total);
#ifndef ICPMI_NN_TIMING
    if (use_win && blockIdx.x == 0 && threadIdx.x == 0) st->dbg[win_hit ? 12 : 13] += 1ull; // diagnostics: iterations served by the window / by the full level 0
#endif
    if (total == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { st->n_valid = 0; st->error = ICPMI_ERR_NO_OUTLIER_TO_FILTER; st->done = 1; }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { st->sel_prefix_l[0] = prefix; st->sel_rank_l[0] = rem; st->n_valid = total; }
    // only the elements under the selected 16-bit prefix contribute (a few hundred): no contention
    auto add = [&](float v) {
        if (!(v != INFINITY && v > 0.f)) return;
        const unsigned bits = __float_as_uint(v);
        if ((bits >> 16) != prefix) return;
        atomicAdd(&hists[ICPMI_S2_C1 + ((bits >> 8) & 255u)], 1u);
        atomicAdd(&hists[ICPMI_S2_F1 + ICPMI_S2_FIDX(bits & 0xffffu)], 1u);
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) add(pv[u]);
    for (int64_t i = i0 + PF * stride; i < count; i += stride) add(d2[i]);
}

// ---------------------------------------------------------------------------------------------
// VarTrimmedDistOutlierFilter (optimizeInlierRatio, Phillips et al. 2007): the valid d2 sorted (radix sort of the bit
// patterns, octree.hip), their running sum in double, FRMS(i) = cum(i) / ((i + 1) ((i + 1) / N)^(2 lambda)) minimised over
// minEl <= i < min(maxEl, V); the limit is then the quantile at i_min / N read straight from the sorted array.
//   vt_keys -> radix_sort_pairs -> vt_chunk_sums -> vt_chunk_offsets -> vt_frms -> vt_pick        (a rare chain: not batched)
// ---------------------------------------------------------------------------------------------
constexpr int VT_CHUNK = 2048; // elements per workgroup of the scan (256 threads x 8)

__global__ __launch_bounds__(256) void vt_keys_kernel(const float* __restrict__ d2, int64_t count, IcpState* __restrict__ st,
                                                      unsigned long long* __restrict__ keys, unsigned* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0 && !st->done) nn_stamp_close(st);
    const float v = i < count ? d2[i] : INFINITY;
    const bool valid = v != INFINITY && v > 0.f;
    if (i < count) { keys[i] = valid ? (unsigned long long)__float_as_uint(v) : 0xffffffffull; vals[i] = 0u; } // invalid entries sort to the end
    __shared__ unsigned cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const unsigned long long b = __ballot(valid);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt, (unsigned)__popcll(b));
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(&st->vt_valid, cnt);
}

__device__ __forceinline__ double vt_value(const unsigned long long* __restrict__ sorted, int64_t i, int64_t V)
{
    return i < V ? (double)__uint_as_float((unsigned)sorted[i]) : 0.0;
}

__global__ __launch_bounds__(256) void vt_chunk_sums_kernel(const unsigned long long* __restrict__ sorted, const IcpState* __restrict__ st,
                                                            double* __restrict__ sums)
{
    const int64_t V = st->vt_valid;
    const int64_t base = (int64_t)blockIdx.x * VT_CHUNK + threadIdx.x * 8;
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) s += vt_value(sorted, base + e, V);
    __shared__ double sh[256];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = sh[0];
}

// one workgroup: sums[b] -> sum of the chunks before b, in chunk order (tiles of 1024 through LDS; lane 0 adds them up in order)
__global__ __launch_bounds__(256) void vt_chunk_offsets_kernel(double* __restrict__ sums, int nchunks)
{
    __shared__ double sh[1024];
    __shared__ double carry;
    if (threadIdx.x == 0) carry = 0.0;
    for (int base = 0; base < nchunks; base += 1024) {
        __syncthreads();
        for (int i = threadIdx.x; i < 1024; i += 256) sh[i] = base + i < nchunks ? sums[base + i] : 0.0;
        __syncthreads();
        if (threadIdx.x == 0) {
            double run = carry;
            const int lim = nchunks - base < 1024 ? nchunks - base : 1024;
            for (int i = 0; i < lim; ++i) { const double v = sh[i]; sh[i] = run; run += v; }
            carry = run;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 1024; i += 256) if (base + i < nchunks) sums[base + i] = sh[i];
    }
}

__global__ __launch_bounds__(256) void vt_frms_kernel(const unsigned long long* __restrict__ sorted, int64_t count, const IcpState* __restrict__ st,
                                                      const double* __restrict__ offsets, long long min_el, long long max_el, float lambda,
                                                      double* __restrict__ best_val, long long* __restrict__ best_idx)
{
    const int64_t V = st->vt_valid;
    const int64_t hi = max_el < V ? max_el : V;
    const int64_t base = (int64_t)blockIdx.x * VT_CHUNK + threadIdx.x * 8;
    double v[8], s = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = vt_value(sorted, base + e, V); s += v[e]; }
    __shared__ double sh[256];
    __shared__ long long shi[256];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) { // inclusive scan of the thread totals
        const double add = threadIdx.x >= off ? sh[threadIdx.x - off] : 0.0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    double cum = offsets[blockIdx.x] + (sh[threadIdx.x] - s);
    __syncthreads();
    double bv = INFINITY; long long bi = -1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        cum += v[e];
        if (i >= min_el && i < hi) {
            const double ids = (double)(i + 1), ratio = ids / (double)count;
            const double frms = cum / (ids * pow(ratio, 2.0 * (double)lambda));
            if (bi < 0 || frms < bv) { bv = frms; bi = i; }
        }
    }
    sh[threadIdx.x] = bv; shi[threadIdx.x] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) { // first minimum: smaller value, or the same value at a smaller rank
        if (threadIdx.x < off) {
            const double ov = sh[threadIdx.x + off]; const long long oi = shi[threadIdx.x + off];
            const long long mi = shi[threadIdx.x];
            if (oi >= 0 && (mi < 0 || ov < sh[threadIdx.x] || (ov == sh[threadIdx.x] && oi < mi))) { sh[threadIdx.x] = ov; shi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { best_val[blockIdx.x] = sh[0]; best_idx[blockIdx.x] = shi[0]; }
}

__global__ __launch_bounds__(256) void vt_pick_kernel(const unsigned long long* __restrict__ sorted, int64_t count, IcpState* __restrict__ st,
                                                      const double* __restrict__ best_val, const long long* __restrict__ best_idx, int nchunks,
                                                      long long min_el, int filter_slot)
{
    __shared__ double sh[256];
    __shared__ long long shi[256];
    double bv = INFINITY; long long bi = -1;
    for (int b = threadIdx.x; b < nchunks; b += 256) {
        const double ov = best_val[b]; const long long oi = best_idx[b];
        if (oi >= 0 && (bi < 0 || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    sh[threadIdx.x] = bv; shi[threadIdx.x] = bi;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            const double ov = sh[threadIdx.x + off]; const long long oi = shi[threadIdx.x + off];
            const long long mi = shi[threadIdx.x];
            if (oi >= 0 && (mi < 0 || ov < sh[threadIdx.x] || (ov == sh[threadIdx.x] && oi < mi))) { sh[threadIdx.x] = ov; shi[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const unsigned V = st->vt_valid;
    st->vt_valid = 0; // for the next iteration's count
    if (st->done) return;
    if (V == 0) { st->error = ICPMI_ERR_NO_OUTLIER_TO_FILTER; st->done = 1; return; }
    long long best = shi[0] >= 0 ? shi[0] : min_el;
    const float ratio = (float)best / (float)count;
    st->vt_ratio = ratio;
    unsigned r; // getDistsQuantile(ratio) over the V valid entries
    if (ratio == 1.0f) r = V - 1;
    else { r = (unsigned)((float)V * ratio); if (r > V - 1) r = V - 1; }
    st->limits[filter_slot] = __uint_as_float((unsigned)sorted[r]);
}

} // namespace

// scratch of the VarTrimmedDist passes (operator scratch slots 0..4, shared with the map-side operators: never live at the
// same time on one handle); reserved before a capture starts, looked up again -- same pointers -- when the passes are enqueued
struct VtBuffers { unsigned long long* keys; unsigned* vals; unsigned* tab; double* sums; double* best_val; long long* best_idx; int nchunks; };
static bool chain_has_vartrimmed(const LoopCfg& lc)
{
    for (int f = 0; f < lc.n_out; ++f) if (lc.out_type[f] == ICPMI_OUT_VARTRIMMEDDIST) return true;
    return false;
}
static icpmi_status vt_buffers(icpmi_ctx* c, int64_t count, VtBuffers* b)
{
    b->nchunks = (int)((count + VT_CHUNK - 1) / VT_CHUNK);
    b->keys = scratch_get<unsigned long long>(c, 0, (size_t)2 * count + 2);
    b->vals = scratch_get<unsigned>(c, 1, (size_t)2 * count + 2);
    b->tab = scratch_get<unsigned>(c, 2, radix_sort_tab_words(count, 32));
    b->sums = scratch_get<double>(c, 3, (size_t)2 * b->nchunks + 2);
    b->best_idx = scratch_get<long long>(c, 4, (size_t)b->nchunks + 1);
    if (!b->keys || !b->vals || !b->tab || !b->sums || !b->best_idx) return ICPMI_ERR_HIP;
    b->best_val = b->sums + b->nchunks + 1;
    return ICPMI_OK;
}

icpmi_status selection_reserve(icpmi_ctx* c, const LoopCfg& lc, int64_t count)
{
    VtBuffers vb;
    return chain_has_vartrimmed(lc) ? vt_buffers(c, count, &vb) : ICPMI_OK;
}

void enqueue_selection(icpmi_ctx* c, const LoopCfg& lc, int64_t count, const BatchArgs& ba, const NnOutcome& nn, bool legacy)
{
    const int slot = legacy ? -2 : fused_filter_slot(lc);
    int hb = (int)std::min<int64_t>((count + 2047) / 2048, 256);
    if (hb < 1) hb = 1;
    // RobustOutlierFilter{scaleEstimator: mad}: scale = sqrt(median |d2 - median(d2)|) -- two more selections on the legacy bins
    // (disjoint from the fused levels), on the single-registration path only (a batch with such a chain runs reading by reading)
    for (int f = 0; f < lc.n_out; ++f) {
        if (lc.out_type[f] != ICPMI_OUT_ROBUST) continue;
        const int se = (lc.out_iparam[f] >> 4) & 15;
        const int nb = (int)lc.out_param2[f];
        if (se == ICPMI_SCALE_MAD) {
            for (int dest = 1; dest <= 2; ++dest) {
#define MAD_PASS(P) \
                if (dest == 1) hipLaunchKernelGGL((sel_hist_kernel<P, 1>), dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, c->d_selhist, nb); \
                else hipLaunchKernelGGL((sel_hist_kernel<P, 2>), dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, c->d_selhist, nb); \
                hipLaunchKernelGGL(sel_scan_kernel<P>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, -1.f, f, 0, 0.f, dest, nb);
                MAD_PASS(0) MAD_PASS(1) MAD_PASS(2)
#undef MAD_PASS
            }
        } else if (se == ICPMI_SCALE_BERG) {
            // iteration 1: the median of the finite positive d2 on the legacy bins; later iterations: the last scan kernel alone does the recurrence
#define BERG_PASS(P) \
            hipLaunchKernelGGL((sel_hist_kernel<P, 3>), dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, c->d_selhist, nb); \
            hipLaunchKernelGGL(sel_scan_kernel<P>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, 0.5f, f, 0, lc.out_param[f], 3, nb);
            BERG_PASS(0) BERG_PASS(1) BERG_PASS(2)
#undef BERG_PASS
        } else if (se == ICPMI_SCALE_STD) {
            double* part = reinterpret_cast<double*>(c->d_selhist + ICPMI_SEL_BINS); // 256 doubles between the legacy bins and the fused levels
            static_assert(ICPMI_SEL_BINS + 512 <= ICPMI_S2_C0, "partials of the std estimator fit in front of the fused histograms");
            hipLaunchKernelGGL(std_part_kernel<0>, dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, part, nb);
            hipLaunchKernelGGL(std_tail_kernel<0>, dim3(1), dim3(256), 0, c->stream, c->d_state, part, hb, count, nb);
            hipLaunchKernelGGL(std_part_kernel<1>, dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, part, nb);
            hipLaunchKernelGGL(std_tail_kernel<1>, dim3(1), dim3(256), 0, c->stream, c->d_state, part, hb, count, nb);
        }
    }
    for (int f = 0; f < lc.n_out; ++f) {
        if (lc.out_type[f] != ICPMI_OUT_VARTRIMMEDDIST) continue;
        VtBuffers vb;
        if (vt_buffers(c, count, &vb) != ICPMI_OK) return; // reserved by the caller: cannot fail here
        const long long min_el = (long long)floorf(lc.out_param[f] * (float)count), max_el = (long long)floorf(lc.out_param2[f] * (float)count);
        hipLaunchKernelGGL(vt_keys_kernel, dim3((int)((count + 255) / 256)), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, vb.keys, vb.vals);
        int half = 0;
        if (radix_sort_pairs(c, vb.keys, vb.vals, count, 32, vb.tab, &half) != ICPMI_OK) return;
        const unsigned long long* sorted = vb.keys + (half ? count : 0);
        hipLaunchKernelGGL(vt_chunk_sums_kernel, dim3(vb.nchunks), dim3(256), 0, c->stream, sorted, c->d_state, vb.sums);
        hipLaunchKernelGGL(vt_chunk_offsets_kernel, dim3(1), dim3(256), 0, c->stream, vb.sums, vb.nchunks);
        hipLaunchKernelGGL(vt_frms_kernel, dim3(vb.nchunks), dim3(256), 0, c->stream, sorted, count, c->d_state, (const double*)vb.sums, min_el, max_el,
                           lc.out_param3[f], vb.best_val, vb.best_idx);
        hipLaunchKernelGGL(vt_pick_kernel, dim3(1), dim3(256), 0, c->stream, sorted, count, c->d_state, (const double*)vb.best_val,
                           (const long long*)vb.best_idx, vb.nchunks, min_el, f);
    }
    if (slot >= 0) {
        // fused chain: hist0 -> [scan0 + hist1] -> [scan1 + hist2]; scan2 happens inside the accumulation kernel
        const float quant = lc.out_type[slot] == ICPMI_OUT_MEDIANDIST ? 0.5f : lc.out_param[slot];
        if (!nn.built_hist0) {
            // 4096 matches per workgroup: every workgroup flushes its LDS table with global atomics, fewer of them win (knn 6, 600 k
            // matches: 1024 per workgroup -6 %, 2048 baseline, 4096 +0.8 %, 8192 -4 %)
            int hb0 = (int)std::min<int64_t>((count + 4095) / 4096, 256);
            if (hb0 < 1) hb0 = 1;
            hipLaunchKernelGGL(sel2_hist0_kernel, dim3(hb0, ba.nscan), dim3(256), 0, c->stream, c->d_d2, ba, lc.k, c->d_state, c->d_selhist, quant,
                               nn.built_win ? 1 : 0);
        }
        int hb2 = (int)std::min<int64_t>((count + 511) / 512, 512);
        if (hb2 < 1) hb2 = 1;
        hipLaunchKernelGGL(sel2_scan_hist_kernel, dim3(hb2, ba.nscan), dim3(256), 0, c->stream, c->d_d2, ba, lc.k, c->d_state, c->d_selhist, quant,
                           (nn.built_win && !nn.built_hist0) ? 1 : 0);
        return;
    }
    for (int f = 0; f < lc.n_out; ++f) {
        const int type = lc.out_type[f];
        if (type != ICPMI_OUT_TRIMMEDDIST && type != ICPMI_OUT_MEDIANDIST) continue;
        const int is_med = type == ICPMI_OUT_MEDIANDIST;
        const float quant = is_med ? 0.5f : lc.out_param[f];
        const float factor = lc.out_param[f];
        hipLaunchKernelGGL((sel_hist_kernel<0, 0>), dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, c->d_selhist, 0);
        hipLaunchKernelGGL(sel_scan_kernel<0>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, quant, f, is_med, factor, 0, 0);
        hipLaunchKernelGGL((sel_hist_kernel<1, 0>), dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, c->d_selhist, 0);
        hipLaunchKernelGGL(sel_scan_kernel<1>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, quant, f, is_med, factor, 0, 0);
        hipLaunchKernelGGL((sel_hist_kernel<2, 0>), dim3(hb), dim3(256), 0, c->stream, c->d_d2, count, c->d_state, c->d_selhist, 0);
        hipLaunchKernelGGL(sel_scan_kernel<2>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, quant, f, is_med, factor, 0, 0);
    }
}
