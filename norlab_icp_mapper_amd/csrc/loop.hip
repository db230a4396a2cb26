// loop.hip -- the device-resident ICP iteration (PM::ICPSequence::operator(), reference call site
// norlab_icp_mapper/Mapper.cpp:213; loop body SURVEY.md B.1):
//     transform (fused into the NN query load) -> kNN -> outlier weights -> pair sums -> solve ->
//     compose -> checkers
// Per iteration the stream carries: the NN kernel (nn.hip), the chain's quantile / scale selections
// on the float bits of d^2 (select.hip), one accumulation kernel and one single-wave solve kernel.
// All decisions (convergence, errors) stay on the device in IcpState; kernels of a finished loop
// exit on st->done.  Behind the loop: the passes over the last iteration's pairs (overlap,
// covariance, residual), which share one walk (walk_pairs) and one ordered double sum.
#include "common.h"
#include "solve.h"
#include <cstring>
#include <type_traits>
#include <vector>

namespace {

// fixed-order sum (halving tree 128 .. 1) of the workgroup's 256 values; the result in every thread
template <class V>
__device__ __forceinline__ V block_tree_sum(V v, V* sh /* 256 */)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) sh[threadIdx.x] += sh[threadIdx.x + h];
        __syncthreads();
    }
    const V r = sh[0];
    __syncthreads();
    return r;
}

// ---------------------------------------------------------------------------------------------
// pair sums (ErrorMinimizer::compute gather + the products of SURVEY.md B.5 / B.6)
// layout of the ICPMI_NV doubles:
//   point-to-plane: [0..20] upper triangle of A row-major, [21..26] b (plane-to-plane: the same slots)
//   point-to-point: [0] sum w, [1..3] sum w p, [4..6] sum w q, [7 + 3c + r] sum w q_r p_c
//   always:         [27] sum w, [28] number of pairs
// ---------------------------------------------------------------------------------------------
// workgroups that take part in the pair sums of `count` matches (the host's acc_blocks): a batch launches the grid of its
// largest reading, every reading uses the workgroups -- and therefore the summation order -- it would use alone
// threads per pair-sum workgroup: k = 1 gives every lane one or two pairs; with k matches per query a 256-thread workgroup left every lane
// ~9 pairs to walk one dependent gather after the other with ONE wave per SIMD to hide it (knn 6: 20 us) -- 1024 threads per workgroup
// keep the number of partials (and the solve's ordered reduction) and give every lane at most three
__host__ __device__ __forceinline__ int acc_threads(int k) { return k > 1 ? 1024 : 256; }
__host__ __device__ __forceinline__ int acc_blocks_dev(int64_t count, int cap, int bt = 256)
{
    const int64_t nb = (count + bt - 1) / bt;
    return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

// a normal's three components (its fourth word is padding: 12 bytes requested, three registers held while the load is in flight)
__device__ __forceinline__ float4 ld_normal(const float4* __restrict__ p)
{
    const float3 v = *reinterpret_cast<const float3*>(p);
    return make_float4(v.x, v.y, v.z, 0.f);
}

// PM: the pair model (common.h: PairModel; lc.pair_model picks the instantiation, enqueue_accumulate_solve)
template <PairModel PM, bool FUSED, bool EXT, int BT>
__global__ __launch_bounds__(BT) void accumulate_kernel(const float4* __restrict__ reading, BatchArgs ba, int acc_cap, LoopCfg lc,
                                                         IcpState* __restrict__ st, const float4* __restrict__ map,
                                                         const float4* __restrict__ normals,
                                                         const float4* __restrict__ read_normals,
                                                         const int* __restrict__ sidx, const float* __restrict__ d2a,
                                                         unsigned* __restrict__ hists,
                                                         int fused_slot, int is_median, float factor,
                                                         const float4* __restrict__ match_pt, const int* __restrict__ qindex,
                                                         const float* __restrict__ ref_scalar, const float4* __restrict__ pnm)
{
    // pnm != nullptr (k > 1, point-to-plane): matched point and its normal sit side by side -- one gather, one 64-byte sector
    // blockIdx.y = reading of a batch (common.h: BatchArgs); a single registration is the batch of one
    // every kernel argument the prologue reads, requested from the kernarg segment in ONE batch (the idiom of nn.hip's prologue)
    asm volatile("" ::"s"(ba.n[blockIdx.y]), "s"(ba.qstride), "s"(acc_cap), "s"(lc.k), "s"(lc.n_out), "s"(lc.out_type[0]), "s"(lc.out_param[0]),
                 "s"(reading), "s"(sidx), "s"(d2a), "s"(match_pt), "s"(qindex), "s"(read_normals), "s"(hists), "s"(st), "s"(map), "s"(normals),
                 "s"(pnm), "s"(fused_slot), "s"(is_median), "s"(factor));
    const int n = ba.n[blockIdx.y];
    const int nbe = acc_blocks_dev((int64_t)n * lc.k, acc_cap, BT);
    if ((int)blockIdx.x >= nbe) return;
    {
        const size_t qo = (size_t)blockIdx.y * (size_t)ba.qstride;
        reading += qo; sidx += qo * lc.k; d2a += qo * lc.k;
        if (match_pt) match_pt += qo;
        if (qindex) qindex += qo;
        if (read_normals) read_normals += qo;
        hists += (size_t)blockIdx.y * ICPMI_SELHIST_WORDS;
        st += blockIdx.y;
    }
    // `reading`, sidx, d2a (and match_pt, the matched map points kept by the NN kernel) share one
    // order: the caller's, or -- qindex != nullptr -- the tile-sorted query order of the k = 1 loop,
    // where qindex maps a slot back to the caller's index (needed for reading descriptors only).
    // The first two (k > 1: three) elements of every lane are requested before anything else, behind the
    // loop header (hdr_load: one dword per lane) and in front of the level-1 coarse counts: one trip.
    const int64_t count = (int64_t)n * lc.k;
    const int64_t stride = (int64_t)nbe * BT;                                // (of the clears below: every thread of the reading's grid)
    const int64_t gtid = (int64_t)blockIdx.x * BT + threadIdx.x;
    // r4: a workgroup takes a CONTIGUOUS run of pairs, and the runs go to the XCDs the way the NN kernel hands out its queries
    // (workgroup b runs on XCD b % 8; XCD x gets the x-th eighth of the tile-sorted pairs): the gathers of an XCD -- matched points,
    // normals -- fall into one eighth of the map instead of all of it, inside a 4 MB L2.  ICPMI_ACC_STRIDED: the r1-r3 strided sweeps.
#ifdef ICPMI_ACC_STRIDED
    const int64_t estep = stride;
    const int64_t e_first = gtid, e_end = count;
#else
    const int64_t estep = BT;
    const int wgc = (nbe & 7) == 0 ? (int)(blockIdx.x & 7) * (nbe >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    const int64_t per_wg = (count + nbe - 1) / nbe;
    const int64_t e_first = (int64_t)wgc * per_wg + threadIdx.x;
    const int64_t e_end = ((int64_t)wgc + 1) * per_wg < count ? ((int64_t)wgc + 1) * per_wg : count;
#endif
    // (k > 1: 1024-thread workgroups, one per CU, up to 600 k pairs at knn 6 -- three pairs per lane; a third pair walked AFTER the first two
    // is two more dependent round trips, so all three are requested up front)
    constexpr int PF = BT > 256 ? 3 : 2;
    // the pair models that read the normals of BOTH clouds (plane-to-plane and the symmetric one): same gathers, same two trips
    constexpr bool BOTH_N = PM == PAIR_PLANE_TO_PLANE || PM == PAIR_SYMMETRIC;
    // the photometric term reads the match's (g, I) and the reading's intensity by the caller's index: the same two trips, q and the caller's
    // index with the first (TRIP1_Q: the pair models whose second trip needs them)
    constexpr bool INTENS = PM == PAIR_INTENSITY;
    constexpr bool TRIP1_Q = BOTH_N || INTENS;
    const float4* __restrict__ map_gi = INTENS ? lc.map_gi : nullptr;
    unsigned hw = hdr_load(st);
    float pd2[PF]; int ps[PF]; float4 pr[PF], pq[PF];
    int po[PF]; // plane-to-plane: the caller's index of the reading point, whose normal the second trip fetches
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int64_t e = e_first + u * estep;
        const bool in = e < e_end;
        pd2[u] = in ? ld_stream(d2a + e) : INFINITY;
        ps[u] = in ? ld_stream(sidx + e) : -1;
        pr[u] = ld_stream(reading + (in ? (int)(e / lc.k) : 0));
        if constexpr (TRIP1_Q) po[u] = in ? (qindex ? ld_stream(qindex + (int)(e / lc.k)) : (int)(e / lc.k)) : -1;
        if constexpr (TRIP1_Q) // (every pair arrives at the sums with all four of its gathers: no dependent load behind them)
            pq[u] = (match_pt && in) ? ld_stream(match_pt + e) : (ps[u] >= 0 ? (pnm ? pnm[2 * (size_t)ps[u]] : map[ps[u]]) : make_float4(0.f, 0.f, 0.f, 0.f));
        else
            pq[u] = (match_pt && in) ? ld_stream(match_pt + e) : ((pnm && ps[u] >= 0) ? pnm[2 * (size_t)ps[u]] : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    unsigned cv = (FUSED && threadIdx.x < 256) ? hists[ICPMI_S2_C1 + threadIdx.x] : 0u; // same round trip as the elements
    // the join: ONE point for the header and the coarse counts (issued last: the pairs in front of them have arrived with them).  Every
    // field this kernel needs becomes a scalar here, under the full exec mask; the header register is dead after that
    asm volatile("" : "+v"(hw), "+v"(cv));
    const HdrView hv{hw};
    const int done = hv.i(ICPMI_HDR_W(done));
    const unsigned long long t_nn_begin = hv.u64(ICPMI_HDR_W(t_nn_begin));
    const unsigned sel_rank0 = hv.u(ICPMI_HDR_W(sel_rank_l)), sel_prefix0 = hv.u(ICPMI_HDR_W(sel_prefix_l));
    float T[16]; // the pose stays in scalar registers across the pair loop
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = hv.f(ICPMI_HDR_W(T_iter) + i);
    // second round trip, overlapping the fine-histogram read of the selection scan: the matched normals
    // (plane-to-plane: ... and the reading's own normals, by the caller's index that arrived with the first trip)
    constexpr bool USES_N = pair_reads_map_normals(PM);
    float4 pn[PF], prn[PF];
    float pip[PF]; // the photometric term: the reading point's intensity (prn carries the match's (g, I) there)
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        prn[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        pip[u] = 0.f;
        if constexpr (INTENS) { // (a missing channel or row never gets here -- api.hip refuses the call; NaN would leave the geometric part)
            pn[u] = ps[u] >= 0 ? (pnm ? pnm[2 * (size_t)ps[u] + 1] : normals[ps[u]]) : make_float4(0.f, 0.f, 0.f, 0.f);
            prn[u] = (map_gi && ps[u] >= 0) ? map_gi[ps[u]] : make_float4(0.f, 0.f, 0.f, NAN);
            pip[u] = (lc.read_intensity && po[u] >= 0) ? lc.read_intensity[po[u]] : NAN;
        } else if constexpr (BOTH_N) {
            pn[u] = ps[u] >= 0 ? ld_normal(pnm ? pnm + 2 * (size_t)ps[u] + 1 : normals + ps[u]) : make_float4(0.f, 0.f, 0.f, 0.f);
            if (po[u] >= 0) prn[u] = ld_normal(read_normals + po[u]);
        } else {
            pn[u] = (USES_N && ps[u] >= 0) ? (pnm ? pnm[2 * (size_t)ps[u] + 1] : normals[ps[u]]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if (done) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) nn_stamp_close(st, t_nn_begin);
    // The lane exchanges of this kernel run in registers (common.h: wave_incl_scan, lane_xor) except in the two instantiations that spill more
    // with them than with the shuffles (profiles/tail_dpp_isa_diff.txt): the same partners and operand order, the same bits either way.
    constexpr bool REG_LANES = !(FUSED && EXT && BT == 1024 && (PM == PAIR_PLANE_TO_PLANE || PM == PAIR_SYMMETRIC));
    float fused_limit = 0.f;
    if (FUSED) {
        // scan of level 1: the selected element's bit pattern is prefix(16) | bin(16)
        __shared__ unsigned shsel[16];
        unsigned bin, rem, total;
        block_find_rank_2tier<1, REG_LANES>(cv, hists + ICPMI_S2_F1, false, 0.f, sel_rank0, shsel, bin, rem, total);
        const float q = __uint_as_float((sel_prefix0 << 16) | bin);
        fused_limit = is_median ? factor * q : q;
        if (blockIdx.x == 0 && threadIdx.x == 0) st->limits[fused_slot] = fused_limit;
        // level 0 is dead (its only reader ran in the previous kernel): clear it for the next iteration
#if ICPMI_WT_CLEAR
        clear_words_wt(hists + ICPMI_S2_C0, ICPMI_S2_COPIES * 256 + ICPMI_S2_FCOPIES * 65536, gtid, stride);
        if (lc.k > 1) clear_words_wt(hists + ICPMI_S2_WIN, 2 * ICPMI_WIN_U64, gtid, stride);
#else
        for (int64_t i = gtid; i < ICPMI_S2_COPIES * 256 + ICPMI_S2_FCOPIES * 65536; i += stride) hists[ICPMI_S2_C0 + i] = 0;
        // ... and so is the speculative window of the k > 1 loop (its readers ran in the two kernels before this one)
        if (lc.k > 1) for (int64_t i = gtid; i < 2 * ICPMI_WIN_U64; i += stride) hists[ICPMI_S2_WIN + i] = 0;
#endif
    }
    constexpr int NVAL = USES_N ? 27 : (PM == PAIR_POINT_TO_POINT ? 16 : 0);
    double acc[NVAL > 0 ? NVAL : 1];
#pragma unroll
    for (int i = 0; i < (NVAL > 0 ? NVAL : 1); ++i) acc[i] = 0.0;
    double wsum = 0.0, cnt = 0.0;
    double b2d[3] = {0.0, 0.0, 0.0}; // force2D: b of the 2-D residual (EXT variant only)
    // BOTH_N: the caller hands over everything the pair needs -- q, n_q, the reading's normal and its caller's index okept
    auto pair = [&](int64_t e, float d2, int s, float4 r, float4 qkept, float4 nkept, bool have_n, float4 rnkept, int okept, float ipkept) {
        if (d2 == INFINITY) return;
        const int qi = (int)(e / lc.k);
        float w;
        if (EXT) {
            // the filters that read the pair itself: original index of the matched point (its .w), point-to-plane residual
            const float3 pe = xf_point(T, r.x, r.y, r.z, r.w);
            const float4 qe = (TRIP1_Q || match_pt || (pnm && have_n)) ? qkept : (pnm ? pnm[2 * (size_t)s] : map[s]);
            float plane2 = 0.f;
            if (normals) {
                const float4 ne = TRIP1_Q || (have_n && USES_N) ? nkept : (pnm ? pnm[2 * (size_t)s + 1] : normals[s]);
                const float dx = pe.x - qe.x, dy = pe.y - qe.y, dz = pe.z - qe.z;
                const float dot = dx * ne.x + dy * ne.y + dz * ne.z;
                plane2 = dot * dot;
            }
            w = match_weight<true>(lc, st, d2, T, read_normals, TRIP1_Q ? okept : (qindex ? qindex[qi] : qi), normals, s, FUSED ? fused_slot : -1, fused_limit,
                                   ref_scalar, __float_as_int(qe.w), plane2, BOTH_N ? &rnkept : nullptr);
        } else w = match_weight(lc, st, d2, T, read_normals, TRIP1_Q ? okept : (qindex ? qindex[qi] : qi), normals, s, FUSED ? fused_slot : -1, fused_limit,
                                nullptr, 0, 0.f, BOTH_N ? &rnkept : nullptr);
        if (w == 0.f) return;
        wsum += w; cnt += 1.0;
        if (PM == PAIR_IDENTITY) return;
        const float3 p = xf_point(T, r.x, r.y, r.z, r.w);
        const float4 q = (TRIP1_Q || match_pt || (pnm && have_n)) ? qkept : (pnm ? pnm[2 * (size_t)s] : map[s]);
        if constexpr (PM == PAIR_POINT_TO_POINT) {
            const double dw = w;
            acc[0] += dw;
            acc[1] += dw * p.x; acc[2] += dw * p.y; acc[3] += dw * p.z;
            acc[4] += dw * q.x; acc[5] += dw * q.y; acc[6] += dw * q.z;
            const double wq[3] = {dw * q.x, dw * q.y, dw * q.z};
            const float pc[3] = {p.x, p.y, p.z};
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) acc[7 + 3 * c + rr] += wq[rr] * pc[c];
        } else if constexpr (PM == PAIR_POINT_TO_PLANE) {
            const float4 nn = have_n ? nkept : (pnm ? pnm[2 * (size_t)s + 1] : normals[s]);
            // per-pair quantities in float exactly as the oracle (and Eigen) form them
            const float F[6] = {p.y * nn.z - p.z * nn.y, p.z * nn.x - p.x * nn.z, p.x * nn.y - p.y * nn.x, nn.x, nn.y, nn.z};
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float dot = dx * nn.x + dy * nn.y + dz * nn.z;
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double wf = (double)w * F[a];
#pragma unroll
                for (int b = a; b < 6; ++b) acc[idx++] += wf * F[b];
                acc[21 + a] -= wf * dot;
            }
            if (EXT && lc.force_2d) {
                const float dot2 = dx * nn.x + dy * nn.y; // upstream drops the z row of the features and of the normals
#pragma unroll
                for (int a = 0; a < 3; ++a) b2d[a] -= ((double)w * F[2 + a]) * dot2;
            }
        } else if constexpr (PM == PAIR_INTENSITY) {
            // joint geometric + photometric point-to-plane: two rank-1 updates per pair into the point-to-plane slots,
            // A += w (lambda F_G F_G^T + (1 - lambda) F_I F_I^T), b -= w (lambda F_G r_G + (1 - lambda) F_I r_I).  The geometric terms are the
            // point-to-plane branch's, bit for bit; per-pair terms in float, the weight's products and the sums in double
            const float4 nn = nkept, gi = rnkept;
            const float wi = lc.intensity_w, lam = 1.f - wi;
            const float F[6] = {p.y * nn.z - p.z * nn.y, p.z * nn.x - p.x * nn.z, p.x * nn.y - p.y * nn.x, nn.x, nn.y, nn.z};
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float dot = dx * nn.x + dy * nn.y + dz * nn.z;
            const double wg = (double)w * (double)lam;
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double wf = wg * F[a];
#pragma unroll
                for (int b = a; b < 6; ++b) acc[idx++] += wf * F[b];
                acc[21 + a] -= wf * dot;
            }
            // a pair whose I_p or I_q is not finite adds the geometric part only
            if (fabsf(gi.w) < INFINITY && fabsf(ipkept) < INFINITY) {
                // m = g - n (g . n): the gradient's part in the match's plane; p' = p - n r_G: the reading point's foot on that plane
                const float gn = gi.x * nn.x + gi.y * nn.y + gi.z * nn.z;
                const float mx = gi.x - nn.x * gn, my = gi.y - nn.y * gn, mz = gi.z - nn.z * gn;
                const float ex = dx - nn.x * dot, ey = dy - nn.y * dot, ez = dz - nn.z * dot;
                const float ri = (gi.w + (gi.x * ex + gi.y * ey + gi.z * ez)) - ipkept;
                const float G[6] = {p.y * mz - p.z * my, p.z * mx - p.x * mz, p.x * my - p.y * mx, mx, my, mz};
                const double wp = (double)w * (double)wi;
                idx = 0;
#pragma unroll
                for (int a = 0; a < 6; ++a) {
                    const double wf = wp * G[a];
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[idx++] += wf * G[b];
                    acc[21 + a] -= wf * ri;
                }
            }
        } else if constexpr (PM == PAIR_PLANE_TO_PLANE) {
            // generalized ICP with plane-regularised covariances (common.h: gicp_pair_sums): M = (C(n_q) + C(R n_x))^-1, C(n) = I - (1 - eps) n n^T
            const float4 nq = nkept, rn = rnkept;
            const float g = 1.f - lc.plane_eps;
            const float3 uq = unit_or_zero(nq.x, nq.y, nq.z);
            const float3 up = unit_or_zero(fmaf(T[8], rn.z, fmaf(T[4], rn.y, T[0] * rn.x)), fmaf(T[9], rn.z, fmaf(T[5], rn.y, T[1] * rn.x)),
                                           fmaf(T[10], rn.z, fmaf(T[6], rn.y, T[2] * rn.x)));
            // S = C(n_q) + C(n_p), symmetric: xx xy xz yy yz zz
            const float sxx = 2.f - g * (uq.x * uq.x + up.x * up.x), syy = 2.f - g * (uq.y * uq.y + up.y * up.y), szz = 2.f - g * (uq.z * uq.z + up.z * up.z);
            const float sxy = -g * (uq.x * uq.y + up.x * up.y), sxz = -g * (uq.x * uq.z + up.x * up.z), syz = -g * (uq.y * uq.z + up.y * up.z);
            gicp_pair_sums<true>(acc, sxx, sxy, sxz, syy, syz, szz, p, make_float3(p.x - q.x, p.y - q.y, p.z - q.z), (double)w);
        } else if constexpr (PM == PAIR_SYMMETRIC) {
            // symmetric point-to-plane in its rotated-normals form (Rusinkiewicz 2019): the point-to-plane branch above with the
            // pair normal n_s = (|c| u_q + c u_p) / 2, c = u_q . u_p -- continuous in both normals, and the sign of either cancels bit for bit
            const float4 nq = nkept, rn = rnkept;
            const float3 uq = unit_or_zero(nq.x, nq.y, nq.z);
            const float3 up = unit_or_zero(fmaf(T[8], rn.z, fmaf(T[4], rn.y, T[0] * rn.x)), fmaf(T[9], rn.z, fmaf(T[5], rn.y, T[1] * rn.x)),
                                           fmaf(T[10], rn.z, fmaf(T[6], rn.y, T[2] * rn.x)));
            const bool hq = uq.x != 0.f || uq.y != 0.f || uq.z != 0.f, hp = up.x != 0.f || up.y != 0.f || up.z != 0.f;
            const float c = uq.x * up.x + uq.y * up.y + uq.z * up.z, ac = fabsf(c);
            // no surface model on one side: the other side's normal alone (reading side: this IS point-to-plane); on neither: u_q = 0, nothing is added
            const float3 nn = !hp ? uq : (!hq ? up : make_float3(0.5f * (ac * uq.x + c * up.x), 0.5f * (ac * uq.y + c * up.y), 0.5f * (ac * uq.z + c * up.z)));
            const float F[6] = {p.y * nn.z - p.z * nn.y, p.z * nn.x - p.x * nn.z, p.x * nn.y - p.y * nn.x, nn.x, nn.y, nn.z};
            const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
            const float dot = dx * nn.x + dy * nn.y + dz * nn.z;
            int idx = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double wf = (double)w * F[a];
#pragma unroll
                for (int b = a; b < 6; ++b) acc[idx++] += wf * F[b];
                acc[21 + a] -= wf * dot;
            }
        }
    };
#pragma unroll
    for (int u = 0; u < PF; ++u) pair(e_first + u * estep, pd2[u], ps[u], pr[u], pq[u], pn[u], true, prn[u], TRIP1_Q ? po[u] : 0, pip[u]);
    if constexpr (BOTH_N) {
        for (int64_t e = e_first + PF * estep; e < e_end; e += estep) { // (past a full grid: the four gathers of a pair requested together)
            const float d2 = d2a[e];
            const int s = sidx[e], qi = (int)(e / lc.k), oi = qindex ? qindex[qi] : qi;
            if (s < 0) continue; // (no match: d2 is +inf)
            const float4 r = reading[qi], q = match_pt ? match_pt[e] : (pnm ? pnm[2 * (size_t)s] : map[s]);
            const float4 nq = ld_normal(pnm ? pnm + 2 * (size_t)s + 1 : normals + s), rn = ld_normal(read_normals + oi);
            pair(e, d2, s, r, q, nq, true, rn, oi, 0.f);
        }
    } else if constexpr (INTENS) {
        for (int64_t e = e_first + PF * estep; e < e_end; e += estep) { // (likewise: everything a pair reads is requested together)
            const float d2 = d2a[e];
            const int s = sidx[e], qi = (int)(e / lc.k), oi = qindex ? qindex[qi] : qi;
            if (s < 0) continue; // (no match: d2 is +inf)
            const float4 r = reading[qi], q = match_pt ? match_pt[e] : (pnm ? pnm[2 * (size_t)s] : map[s]);
            const float4 nq = pnm ? pnm[2 * (size_t)s + 1] : normals[s];
            const float4 gi = map_gi ? map_gi[s] : make_float4(0.f, 0.f, 0.f, NAN);
            pair(e, d2, s, r, q, nq, true, gi, oi, lc.read_intensity ? lc.read_intensity[oi] : NAN);
        }
    } else {
        for (int64_t e = e_first + PF * estep; e < e_end; e += estep)
            pair(e, d2a[e], sidx[e], reading[(int)(e / lc.k)], match_pt ? match_pt[e] : make_float4(0.f, 0.f, 0.f, 0.f),
                 make_float4(0.f, 0.f, 0.f, 0.f), false, make_float4(0.f, 0.f, 0.f, 0.f), 0, 0.f);
    }
    // ---- workgroup reduction: lane exchanges inside the wave, then LDS across the waves ----
    // (common.h: pair_sums_fold is this fold as a function, for voxel.hip.  Here it stays spelled out, and so do the rank-1 updates above: the EXT
    // instantiations at 1024 threads sit at the 128-VGPR cap, where the inlined helpers order the same operations differently and spill more)
    // Transposed butterfly: at the step with partner lane ^ m every lane hands over the half of its
    // values the partner keeps, so 32 values x 64 lanes fold with 16+8+4+2+1+1 = 32 exchanges instead
    // of 32 x 6.  After the five halving steps lane l holds value bitrev5(l & 31) summed over its
    // 32-lane half; the last exchange joins the halves.  Fixed pattern => deterministic sums.
    __shared__ double sh[BT / 64][ICPMI_NV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double val[ICPMI_NV];
#pragma unroll
    for (int i = 0; i < ICPMI_NV; ++i) val[i] = i < NVAL ? acc[i < NVAL ? i : 0] : 0.0;
    val[27] = wsum; val[28] = cnt;
    if (EXT) { val[29] = b2d[0]; val[30] = b2d[1]; val[31] = b2d[2]; }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const int m = 1 << s;
        const int nkeep = 16 >> s;
        const bool upper = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < nkeep; ++i) {
            const double send = upper ? val[i] : val[i + nkeep];
            const double keep = upper ? val[i + nkeep] : val[i];
            if constexpr (REG_LANES) val[i] = keep + lane_xor_bit(send, m); // (common.h: lane ^ m in registers, no trip through the LDS crossbar)
            else val[i] = keep + __shfl_xor(send, m, 64);
        }
    }
    if constexpr (REG_LANES) val[0] += lane_xor<32>(val[0]);
    else val[0] += __shfl_xor(val[0], 32, 64);
    if (lane < 32) {
        const int idx = ((lane & 1) << 4) | ((lane & 2) << 2) | (lane & 4) | ((lane & 8) >> 2) | ((lane & 16) >> 4);
        sh[wv][idx] = val[0];
    }
    __syncthreads();
    if (threadIdx.x < ICPMI_NV) {
        const int i = threadIdx.x;
        double v = 0.0;
        if (i < NVAL || i == 27 || i == 28 || (EXT && i > 28)) {
            v = sh[0][i] + sh[1][i] + sh[2][i] + sh[3][i];
#pragma unroll
            for (int w2 = 4; w2 < BT / 64; ++w2) v += sh[w2][i]; // fixed order
        }
        // the workgroup's sum joins the iteration's accumulator as two fixed-point limbs (common.h: ICPMI_ACC_*): integer atomics,
        // so the total is the same whatever order the workgroups arrive in
        unsigned long long* acc = reinterpret_cast<unsigned long long*>(hists + ICPMI_S2_ACC);
        if (v != 0.0) {
            if (!(fabs(v) < 0x1p77)) atomicOr(reinterpret_cast<unsigned*>(acc + ICPMI_ACC_FLAG), 1u);
            else {
                const double hi = rint(v * 0x1p-16);
                const double lo = v - hi * 65536.0;                 // exact: a multiple of ulp(v) below 2^15
                const long long H = (long long)hi, Lq = __double2ll_rn(lo * 0x1p40);
                const int cp = blockIdx.x & (ICPMI_ACC_COPIES - 1);
                if (H) atomicAdd(acc + ICPMI_ACC_IDX(cp, i, 0), (unsigned long long)H);
                if (Lq) atomicAdd(acc + ICPMI_ACC_IDX(cp, i, 1), (unsigned long long)Lq);
            }
        }
    }
}

// (r5) the state of a FINISHED registration goes to the host by itself: the first wave of the solve copies IcpState into the handle's pinned
// host block (`mirror` = device address of icpmi_ctx::h_state; null for batches and operators) in front of the progress word that says
// "done" -- loop_run then returns on that word instead of enqueueing a copy and draining the stream (21 - 26 us per registration between
// the flag and the state on the host, `-DICPMI_TAIL_DIAG`).  Loads past the L1 (thread 0 wrote the state a moment ago), plain stores, and
// the word's system-scope release behind them: one wave, one instruction stream.
__device__ __forceinline__ void mirror_state(const IcpState* st, IcpState* mirror)
{
    const unsigned* src = reinterpret_cast<const unsigned*>(st);
    unsigned* dst = reinterpret_cast<unsigned*>(mirror);
    constexpr int W = (int)(sizeof(IcpState) / sizeof(unsigned));
    for (int i = threadIdx.x; i < W; i += 64) dst[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool DEGEN> // (solve.h: solve_serial)
__global__ __launch_bounds__(256) void solve_kernel(IcpState* __restrict__ st, unsigned* __restrict__ hists, int clear, LoopCfg lc,
                                                    float* __restrict__ T_step_out, double* __restrict__ sums_out, unsigned* __restrict__ progress,
                                                    IcpState* __restrict__ mirror)
{
    // blockIdx.x = reading of a batch: one workgroup per registration
    st += blockIdx.x;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(hists + (size_t)blockIdx.x * ICPMI_SELHIST_WORDS + ICPMI_S2_ACC);
    if (progress) progress += blockIdx.x;
    // (r5: the brute pass's queue is emptied here instead of by a one-thread launch of its own behind every NN launch of a chain with an
    //  unbounded maxDist -- the next NN launch starts behind this kernel)
    if (threadIdx.x == 0 && st->hard_count) { st->hard_total += st->hard_count; st->hard_count = 0; }
    if (st->done) { // finished earlier, or an upstream kernel of this iteration raised an error
        if (mirror && threadIdx.x < 64) mirror_state(st, mirror + blockIdx.x); // (the same words again after the first time: harmless)
        if (threadIdx.x == 0) publish_progress(st, progress);
        return;
    }
    solve_body<DEGEN>(st, acc, clear != 0, lc, T_step_out, sums_out);
    if (threadIdx.x == 0 && st->done) st->t_done = (unsigned long long)wall_clock64();
    if (mirror) {
        __syncthreads(); // thread 0's stores to the state are issued
        if (threadIdx.x < 64 && __hip_atomic_load(&st->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) mirror_state(st, mirror + blockIdx.x);
    }
    if (threadIdx.x == 0) publish_progress(st, progress);
}

// ---- scheduled VoxelMatcher handles ---------------------------------------------
// The level word of the header and the report of the handle's device block (common.h: ICPMI_VS_*), set behind init_state: a registration's
// head starts at level 0, a one-pass evaluation (icpmi_minimize_step_normals) at the level it asks for.
__global__ __launch_bounds__(64) void voxel_sched_reset_kernel(IcpState* __restrict__ st, unsigned* __restrict__ sched, unsigned level)
{
    if (threadIdx.x == 0) st->vox_level = level;
    if (threadIdx.x < ICPMI_VS_WORDS - ICPMI_VS_BASE) sched[ICPMI_VS_BASE + threadIdx.x] = 0u;
}

// One wave behind every solve of a scheduled handle.  The solve is the one every chain runs and knows nothing of levels: when a checker
// stops the loop it sets `done`.  This kernel keeps the level's report (iterations, pair count of its first and of its last iteration:
// the same values again on the dead iterations behind the end), and while a level remains and the stop is no error it makes the stop a
// level switch: `done` cleared, the Counter at zero, the Differential checker's history empty, the level raised.  T_iter, iter (the total
// over the levels: what the progress word and the stats carry) and init_q (the Bound checker measures from the registration's start) stay.
// For the host it does what the solve of a one-size handle does itself: the finished state into the mirror, here with the report beside
// it (host_report: 13 words of the progress page), then the word.
__global__ __launch_bounds__(64) void voxel_advance_kernel(IcpState* __restrict__ st, unsigned* __restrict__ sched, int nlevels,
                                                           unsigned* __restrict__ progress, IcpState* __restrict__ mirror,
                                                           unsigned* __restrict__ host_report)
{
    if (threadIdx.x == 0) {
        const int L = (int)(st->vox_level & (ICPMI_MAX_VOXEL_LEVELS - 1));
        const int it = st->iter - (int)sched[ICPMI_VS_BASE];
        const unsigned pairs = (unsigned)st->pairs;
        sched[ICPMI_VS_ITERS + L] = (unsigned)it;
        if (it == 1 && pairs) sched[ICPMI_VS_FIRST + L] = pairs; // (a level whose iteration found no pair did not count it)
        sched[ICPMI_VS_LAST + L] = pairs;
        if (st->done && !st->error && L + 1 < nlevels) {
            st->done = 0; st->stop_reason = 0; st->counter = 0; st->t_done = 0;
            // the history begins EMPTY: the pose carried over is not an entry (include/icpmi.h), so the first step the checker may count is
            // the one between the level's first two poses.  The solve has no such state of its own (init_state leaves one entry), so it is
            // built from states it has: the ring exactly full (hist_n = RING: the level's first pose goes to slot 0 and is measured against
            // slot RING - 1), that slot a pose 1e30 m away (the step against it is finite and far over any threshold), and every stored step
            // +inf.  A window that still holds a step from before the level's second pose then has an infinite mean -- not under the
            // thresholds, and no NaN (inf - inf never forms: the steps are only added) -- and the first window of the level's own steps is
            // the one behind iteration smoothLength + 1.
            constexpr int RING = ICPMI_MAX_SMOOTH + 1; // (solve.h: the ring of solve_serial's Differential checker)
            for (int i = 0; i < RING; ++i) { st->hrot[i] = INFINITY; st->htr[i] = INFINITY; }
            quat_from_T(st->T_iter, st->hq + 4 * (RING - 1));
            for (int r = 0; r < 3; ++r) st->ht[3 * (RING - 1) + r] = 1e30;
            st->hist_n = RING;
            sched[ICPMI_VS_BASE] = (unsigned)st->iter;
            st->vox_level = (unsigned)(L + 1);
        }
    }
    __syncthreads(); // thread 0's stores to the state and the report are issued
    if (__hip_atomic_load(&st->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        if (mirror) mirror_state(st, mirror);
        if (progress && threadIdx.x < 1 + 3 * ICPMI_MAX_VOXEL_LEVELS) {
            const int t = threadIdx.x;
            const unsigned v = t == 0 ? __hip_atomic_load(&st->vox_level, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u
                                      : __hip_atomic_load(sched + ICPMI_VS_ITERS + (t - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            host_report[t] = v;
        }
    }
    if (threadIdx.x == 0) publish_progress(st, progress);
}

// ---- a batch on the voxel path --------------------------------------------------
// blockIdx.x = member: its state, its report block (ICPMI_VS_WORDS dwords behind the descriptor block of the handle's batch block), its
// progress word.  A one-size handle runs the reset too: the pair kernel of a batch reads the level word on every handle.
__global__ __launch_bounds__(64) void voxel_sched_reset_batch_kernel(IcpState* __restrict__ st, unsigned* __restrict__ blocks)
{
    st += blockIdx.x;
    unsigned* __restrict__ sched = blocks + (size_t)(1 + blockIdx.x) * ICPMI_VS_WORDS;
    if (threadIdx.x == 0) st->vox_level = 0u;
    if (threadIdx.x < ICPMI_VS_WORDS - ICPMI_VS_BASE) sched[ICPMI_VS_BASE + threadIdx.x] = 0u;
}

// voxel_advance_kernel for the members of a batch, one wave each: the same report and the same level switch, on the member's own state and
// report block.  No mirror and no host report: a batch reads its states back at the end, and the report blocks with them.
__global__ __launch_bounds__(64) void voxel_advance_batch_kernel(IcpState* __restrict__ st, unsigned* __restrict__ blocks, int nlevels,
                                                                 unsigned* __restrict__ progress)
{
    st += blockIdx.x;
    unsigned* __restrict__ sched = blocks + (size_t)(1 + blockIdx.x) * ICPMI_VS_WORDS;
    if (progress) progress += blockIdx.x;
    if (threadIdx.x == 0) {
        const int L = (int)(st->vox_level & (ICPMI_MAX_VOXEL_LEVELS - 1));
        const int it = st->iter - (int)sched[ICPMI_VS_BASE];
        const unsigned pairs = (unsigned)st->pairs;
        sched[ICPMI_VS_ITERS + L] = (unsigned)it;
        if (it == 1 && pairs) sched[ICPMI_VS_FIRST + L] = pairs;
        sched[ICPMI_VS_LAST + L] = pairs;
        if (st->done && !st->error && L + 1 < nlevels) {
            st->done = 0; st->stop_reason = 0; st->counter = 0; st->t_done = 0;
            // (the history of the new level begins empty: voxel_advance_kernel says how that state is built)
            constexpr int RING = ICPMI_MAX_SMOOTH + 1;
            for (int i = 0; i < RING; ++i) { st->hrot[i] = INFINITY; st->htr[i] = INFINITY; }
            quat_from_T(st->T_iter, st->hq + 4 * (RING - 1));
            for (int r = 0; r < 3; ++r) st->ht[3 * (RING - 1) + r] = 1e30;
            st->hist_n = RING;
            sched[ICPMI_VS_BASE] = (unsigned)st->iter;
            st->vox_level = (unsigned)(L + 1);
        }
        publish_progress(st, progress);
    }
}

__global__ __launch_bounds__(256) void centre_kernel(BatchSrc src, BatchArgs ba, float mx, float my, float mz, float4* __restrict__ out)
{
    // blockIdx.y = reading of a batch: its own source pointer, slice blockIdx.y of `out`
    const int64_t n = ba.n[blockIdx.y];
    const float4* __restrict__ scan = src.p[blockIdx.y];
    out += (size_t)blockIdx.y * (size_t)ba.qstride;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = scan[i];
    // reading moved by T_refMean_dataIn = [I | -mean] through the same fmaf chain as a transform
    out[i] = make_float4(fmaf(-mx, p.w, p.x), fmaf(-my, p.w, p.y), fmaf(-mz, p.w, p.z), p.w);
}

__global__ __launch_bounds__(256) void pad_normals_kernel(const float* __restrict__ n3, int64_t n, float4* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = make_float4(n3[3 * i], n3[3 * i + 1], n3[3 * i + 2], 0.f);
}

// T0_stride: floats between the start poses of the readings (0: every reading starts from the one T0; 16: a table, one pose per reading)
__global__ void init_state_kernel(IcpState* st, const float* T0, unsigned seq, unsigned* progress, const unsigned* seq_src = nullptr,
                                  int T0_stride = 0)
{
    if (threadIdx.x != 0) return;
    st[blockIdx.x].t_start = (unsigned long long)wall_clock64(); // (a head that is not folded into the query sort: this kernel stands for its start)
    init_state_dev(st + blockIdx.x, T0 ? T0 + (size_t)blockIdx.x * T0_stride : nullptr, seq, progress ? progress + blockIdx.x : nullptr,
                   seq_src); // one state per reading of a batch
}

__global__ __launch_bounds__(256) void weights_kernel(int64_t count, LoopCfg lc, const IcpState* __restrict__ st,
                                                      const float4* __restrict__ normals, const float4* __restrict__ read_normals,
                                                      const int* __restrict__ sidx, const float* __restrict__ d2a,
                                                      float* __restrict__ w, const float* __restrict__ ref_scalar)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const int s = sidx[e];
    float wt = 1.f;
    // the chain is evaluated on every entry like upstream (an invalid match has d2 = +inf and fails
    // every "<= limit" test; SurfaceNormal / GenericDescriptor need a valid id, Robust gives an unmatched entry weight 0).
    // This stage entry point gets ORIGINAL ids: the scalar channel is indexed by them directly.
    bool needs_id = false;
    for (int f = 0; f < lc.n_out; ++f) needs_id |= lc.out_type[f] == ICPMI_OUT_SURFACENORMAL || lc.out_type[f] == ICPMI_OUT_GENERICDESCRIPTOR || lc.out_type[f] == ICPMI_OUT_ROBUST;
    if (needs_id && (s < 0 || (lc.ext && d2a[e] == INFINITY))) wt = 0.f;
    else if (lc.ext) wt = match_weight<true>(lc, st, d2a[e], nullptr, read_normals, (int)(e / lc.k), normals, s < 0 ? 0 : s, -1, 0.f, ref_scalar, s < 0 ? 0 : s, 0.f);
    else wt = match_weight(lc, st, d2a[e], nullptr, read_normals, (int)(e / lc.k), normals, s < 0 ? 0 : s);
    w[e] = wt;
}

} // namespace

LoopCfg make_loop_cfg(const icpmi_ctx* c, int fixed_iterations)
{
    LoopCfg lc;
    memset(&lc, 0, sizeof lc);
    const icpmi_config& cfg = c->cfg;
    lc.k = cfg.knn < 1 ? 1 : cfg.knn;
    lc.max_dist = cfg.max_dist;
    lc.maxr2 = squared_radius(cfg.max_dist);
    lc.inv1e = 1.f; lc.err2 = 1.f;
    if (cfg.epsilon_approx && cfg.epsilon > 0.f) { // both rounded to the conservative side (a larger pruning radius, a stricter decision)
        const double e1 = 1.0 + (double)cfg.epsilon;
        lc.inv1e = (float)(1.0 / e1); if ((double)lc.inv1e < 1.0 / e1) lc.inv1e = nextafterf(lc.inv1e, 2.f);
        lc.err2 = (float)(e1 * e1); if ((double)lc.err2 > e1 * e1) lc.err2 = nextafterf(lc.err2, 0.f);
    }
    const int RING_CAP = 16;
    if (std::isfinite(cfg.max_dist) && c->grid.cell > 0.f) {
        const int need = (int)ceilf(cfg.max_dist / c->grid.cell) + 1;
        lc.ring_max = need < RING_CAP ? need : RING_CAP;
    } else lc.ring_max = 6;
    if (lc.ring_max < 1) lc.ring_max = 1;
    // plane-to-plane fills the point-to-plane slots of the sums: every kernel behind the pair sums sees a point-to-plane chain
    const bool gicp = cfg.minimizer == ICPMI_MIN_PLANE_TO_PLANE;
    lc.minimizer = gicp ? ICPMI_MIN_POINT_TO_PLANE : cfg.minimizer;
    lc.n_out = cfg.n_outlier;
    for (int f = 0; f < cfg.n_outlier && f < ICPMI_MAX_OUTLIER; ++f) {
        lc.out_type[f] = cfg.outlier[f].type;
        lc.out_param[f] = cfg.outlier[f].param;
        lc.out_iparam[f] = cfg.outlier[f].iparam;
        lc.out_param2[f] = cfg.outlier[f].param2;
        lc.out_param3[f] = cfg.outlier[f].param3;
        if (lc.out_type[f] == ICPMI_OUT_GENERICDESCRIPTOR || lc.out_type[f] == ICPMI_OUT_ROBUST) lc.ext = 1;
    }
    lc.force_4dof = cfg.force_4dof != 0 && lc.minimizer == ICPMI_MIN_POINT_TO_PLANE;
    lc.is_2d = cfg.is_2d != 0;
    lc.force_2d = (cfg.force_2d != 0 || cfg.is_2d != 0) && cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE;
    if (lc.force_2d) lc.ext = 1;
    if (fixed_iterations > 0) {
        lc.max_iter = fixed_iterations; lc.use_diff = 0; lc.use_bound = 0;
    } else {
        lc.max_iter = cfg.max_iterations;
        lc.use_diff = cfg.use_differential; lc.use_bound = cfg.use_bound;
    }
    lc.min_rot = cfg.min_diff_rot; lc.min_trans = cfg.min_diff_trans;
    lc.smooth = cfg.smooth_length < 1 ? 1 : (cfg.smooth_length > ICPMI_MAX_SMOOTH ? ICPMI_MAX_SMOOTH : cfg.smooth_length);
    lc.max_rot = cfg.max_rot_norm; lc.max_trans = cfg.max_trans_norm;
    // degeneracy-aware solve: only once the handle has the side block (the entry points that run a solve allocate it first: api.hip)
    if (cfg.degeneracy_threshold != 0.f && cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE && c->d_degen.get()) {
        lc.degen = cfg.degeneracy_threshold > 0.f ? ICPMI_DG_CONSTRAIN : ICPMI_DG_REPORT;
        lc.degen_thr = fabsf(cfg.degeneracy_threshold);
        lc.degen_blk = c->d_degen.get();
    }
    // THE place that chooses the pair sums' model; the fields a model owns are set for it alone (the others stay 0 from the memset)
    if (gicp && c->plane_model == ICPMI_PLANE_MODEL_SYMMETRIC) lc.pair_model = PAIR_SYMMETRIC;
    else if (gicp) {
        lc.pair_model = PAIR_PLANE_TO_PLANE;
        lc.plane_eps = c->plane_eps;
    } else if (c->intensity_w > 0.f && cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE && lc.degen == 0) { // (api.hip refuses the term with the degeneracy-aware solve)
        lc.pair_model = PAIR_INTENSITY;
        lc.intensity_w = c->intensity_w;
        lc.map_gi = map_intensity_ready(c) ? c->d_map_gi.get() : nullptr; // (the reading's row: api.hip, intensity_setup)
    } else lc.pair_model = cfg.minimizer == ICPMI_MIN_POINT_TO_PLANE ? PAIR_POINT_TO_PLANE : (cfg.minimizer == ICPMI_MIN_POINT_TO_POINT ? PAIR_POINT_TO_POINT : PAIR_IDENTITY);
    return lc;
}

// Which of the handle's buffers hold the matcher's last output under chain lc; sorted = NnOutcome::out_sorted of that launch (k = 1: with
// the matched points, see nn1_wg_kernel; k > 1: ids and d2).  THE place where this is decided: the pair-sum launch and every pass behind
// the loop read from it.  Before it, the covariance pass took d_normals_sorted and the overlap pass d_read_normals unconditionally; the
// conditional forms here are the same pointers wherever a kernel dereferences them -- the covariance runs for point-to-plane only, which
// api.hip (register_impl) refuses without map normals, and the overlap pass runs with !lc.ext and reads the reading's normals in its
// point-to-plane branch only, for which register_impl sets has_read_normals (a SurfaceNormal filter sets it through chain_setup).
PairView pair_view(const icpmi_ctx* c, const LoopCfg& lc, bool sorted)
{
    PairView v;
    v.reading = sorted ? c->d_qsorted : c->d_reading;
    v.qindex = sorted ? c->d_qindex : nullptr;
    v.sidx = c->d_sidx;
    v.d2 = c->d_d2;
    v.match_pt = (sorted && lc.k == 1) ? c->d_match_pt : nullptr;
    v.map = c->d_map_sorted;
    v.ref_normals = c->has_normals ? c->d_normals_sorted : nullptr;
    v.read_normals = lc.has_read_normals ? c->d_read_normals : nullptr;
    v.ref_scalar = (lc.ext && c->raw_has_scalar) ? c->d_raw_s : nullptr;
    return v;
}

// ---------------------------------------------------------------------------------------------
// ErrorMinimizer::getOverlap() for a reading that carries `simpleSensorNoise` and `normals` (read at Mapper.cpp:219).
// The pairs are the last iteration's error elements: reading point under T_prev, its match, weight != 0.
//   PointToPoint : dists_i = |p - q|, mean over the pairs, count(dists_i < mean + noise_i) / pairs
//   PointToPlane : count(|(p - q) . n_i / |n_i|| < noise_i) / pairs, n_i = the READING's normal under T_prev
// MODE 0: per-workgroup partial sums {pairs, sum of dists} in a fixed order (p2p needs the mean first); MODE 1: the count.
// ---------------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void overlap_kernel(PairView pv, int n, LoopCfg lc, const IcpState* __restrict__ st,
                                                      const float* __restrict__ noise, float mean, double* __restrict__ partial,
                                                      unsigned long long* __restrict__ count)
{
    const float* T = st->T_prev;
    double np = 0.0, sd = 0.0;
    unsigned long long cnt = 0;
    walk_pairs(pv, n, lc, st, T, [&](const PairSlot& a) {
        if (a.w == 0.f) return;
        const bool p2p = lc.minimizer == ICPMI_MIN_POINT_TO_POINT;
        if (MODE == 0) { // (one statement per sum: the sums stay in registers)
            np += 1.0;
            sd += p2p ? (double)sqrtf(fmaf(a.dz, a.dz, fmaf(a.dy, a.dy, a.dx * a.dx))) : 0.0;
        } else if (p2p) {
            const float dist = sqrtf(fmaf(a.dz, a.dz, fmaf(a.dy, a.dy, a.dx * a.dx)));
            if (dist < mean + noise[a.oi]) ++cnt;
        } else {
            const float4 rn = pv.read_normals[a.oi];
            const float nx = fmaf(T[8], rn.z, fmaf(T[4], rn.y, T[0] * rn.x)), ny = fmaf(T[9], rn.z, fmaf(T[5], rn.y, T[1] * rn.x)),
                        nz = fmaf(T[10], rn.z, fmaf(T[6], rn.y, T[2] * rn.x));
            const float nn = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx)));
            const float proj = fmaf(a.dz, nz / nn, fmaf(a.dy, ny / nn, a.dx * (nx / nn)));
            if (fabsf(proj) < noise[a.oi]) ++cnt;
        }
    });
    if (MODE == 0) {
        __shared__ double sh[256];
        const double pairs = block_tree_sum(np, sh), dists = block_tree_sum(sd, sh);
        if (threadIdx.x == 0) { partial[2 * blockIdx.x] = pairs; partial[2 * blockIdx.x + 1] = dists; }
    } else {
        __shared__ unsigned long long shc[256];
        const unsigned long long c = block_tree_sum(cnt, shc);
        if (threadIdx.x == 0 && c) atomicAdd(count, c);
    }
}

icpmi_status loop_sensor_noise_overlap(icpmi_ctx* c, int64_t n, const LoopCfg& lc, bool sorted, float* overlap)
{
    *overlap = -1.f;
    constexpr int NB = 128;
    double* d_part = scratch_get<double>(c, 5, 2 * NB + 2);
    if (!d_part) return ICPMI_ERR_HIP;
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d_part + 2 * NB);
    HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), c->stream));
    const PairView pv = pair_view(c, lc, sorted);
    hipLaunchKernelGGL(overlap_kernel<0>, dim3(NB), dim3(256), 0, c->stream, pv, (int)n, lc, c->d_state, c->d_read_noise, 0.f, d_part, d_cnt);
    double hp[2 * NB];
    if (read_back(c, hp, d_part, sizeof hp) != ICPMI_OK) return ICPMI_ERR_HIP;
    double pairs = 0.0, sum = 0.0;
    for (int b = 0; b < NB; ++b) { pairs += hp[2 * b]; sum += hp[2 * b + 1]; }
    if (!(pairs > 0.0)) return ICPMI_OK;
    const float mean = (float)(sum / pairs);
    hipLaunchKernelGGL(overlap_kernel<1>, dim3(NB), dim3(256), 0, c->stream, pv, (int)n, lc, c->d_state, c->d_read_noise, mean, d_part, d_cnt);
    unsigned long long hc = 0;
    if (read_back(c, &hc, d_cnt, sizeof hc) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipGetLastError());
    *overlap = (float)((double)hc / pairs);
    return ICPMI_OK;
}

// ---------------------------------------------------------------------------------------------
// PointToPlaneWithCovErrorMinimizer::getCovariance() (include/icpmi.h: icpmi_get_covariance has the formula).  Two launches behind the
// loop, outside any graph, over the same pairs as the overlap pass: the last counted iteration's error elements with w > 0, the reading
// under T_prev.  Pass 1: every workgroup sums h h^T and a a^T + b b^T (21 + 21 upper-triangle values) in double and writes its partials;
// pass 2 (one workgroup) adds the partials in a fixed order, factors H and writes Cov.  No atomics: the same bits on every call.
// ---------------------------------------------------------------------------------------------
#define ICPMI_COV_NB 256   // pass-1 workgroups, one per CU (fixed: the summation order must not depend on anything but the pair count)
#define ICPMI_COV_NV 42    // [0..20] H, [21..41] S, upper triangles row-major

// (tx, ty, tz, alpha, beta, gamma) of the last step T_s = T_iter T_prev^-1 (T_prev^-1 = [R^T | -R^T t]), in double
__device__ inline void cov_step_params(const IcpState* st, double* x)
{
    const float* A = st->T_iter;
    const float* P = st->T_prev;
    double R[3][3];
    for (int r = 0; r < 3; ++r)
        for (int cc = 0; cc < 3; ++cc) R[r][cc] = (double)A[r] * P[cc] + (double)A[4 + r] * P[4 + cc] + (double)A[8 + r] * P[8 + cc];
    for (int r = 0; r < 3; ++r) x[r] = (double)A[12 + r] - (R[r][0] * P[12] + R[r][1] * P[13] + R[r][2] * P[14]);
    const double beta = -asin(R[2][0]);
    const double cb = cos(beta);
    x[3] = atan2(R[2][1], R[2][2]);
    x[4] = beta;
    x[5] = atan2(R[1][0] / cb, R[0][0] / cb);
}

__global__ __launch_bounds__(256) void cov_pairs_kernel(PairView pv, int n, LoopCfg lc, const IcpState* __restrict__ st,
                                                        double* __restrict__ partial)
{
    __shared__ double xs[6];
    if (threadIdx.x == 0) cov_step_params(st, xs);
    __syncthreads();
    const double tx = xs[0], ty = xs[1], tz = xs[2], al = xs[3], be = xs[4], ga = xs[5];
    double acc[ICPMI_COV_NV];
#pragma unroll
    for (int i = 0; i < ICPMI_COV_NV; ++i) acc[i] = 0.0;
    walk_pairs(pv, n, lc, st, st->T_prev, [&](const PairSlot& s) {
        if (!(s.w > 0.f)) return;
        const double px = s.p.x, py = s.p.y, pz = s.p.z, qx = s.q.x, qy = s.q.y, qz = s.q.z, nx = s.nm.x, ny = s.nm.y, nz = s.nm.z;
        const double r = sqrt(px * px + py * py + pz * pz), rho = sqrt(qx * qx + qy * qy + qz * qz);
        const double ir = 1.0 / r, irho = 1.0 / rho; // (two double divisions per pair instead of six)
        const double dx = px * ir, dy = py * ir, dz = pz * ir, ux = qx * irho, uy = qy * irho, uz = qz * irho;
        const double cx = dy * nz - dz * ny, cy = dz * nx - dx * nz, cz = dx * ny - dy * nx;
        // L v = v + (alpha, beta, gamma) x v
        const double lpx = px - ga * py + be * pz, lpy = ga * px + py - al * pz, lpz = -be * px + al * py + pz;
        const double ldx = dx - ga * dy + be * dz, ldy = ga * dx + dy - al * dz, ldz = -be * dx + al * dy + dz;
        const double E = nx * (lpx + tx - qx) + ny * (lpy + ty - qy) + nz * (lpz + tz - qz);
        const double Nr = nx * ldx + ny * ldy + nz * ldz;
        const double Nq = -(nx * ux + ny * uy + nz * uz);
        const double ea = E + r * Nr;
        const double h[6] = {nx, ny, nz, r * cx, r * cy, r * cz};
        const double a[6] = {nx * Nr, ny * Nr, nz * Nr, cx * ea, cy * ea, cz * ea};
        const double b[6] = {nx * Nq, ny * Nq, nz * Nq, r * cx * Nq, r * cy * Nq, r * cz * Nq};
        int idx = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j, ++idx) {
                acc[idx] += h[i] * h[j];
                acc[21 + idx] += a[i] * a[j] + b[i] * b[j];
            }
    });
    block_partial_row<ICPMI_COV_NV>(acc, partial + (size_t)blockIdx.x * ICPMI_COV_NV);
}

#define ICPMI_COV_CH 6     // pass 2: six threads per value, each over every sixth workgroup partial
__global__ __launch_bounds__(256) void cov_solve_kernel(const double* __restrict__ partial, int nb, float sigma, float* __restrict__ cov)
{
    __shared__ double tot[ICPMI_COV_NV];
    block_ordered_total<ICPMI_COV_NV, ICPMI_COV_CH, ICPMI_COV_NB>(partial, nb, tot);
    if (threadIdx.x != 0) return;
    double H[6][6], S[6][6], L[6][6], Hi[6][6], M[6][6];
    int idx = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++idx) { H[i][j] = H[j][i] = tot[idx]; S[i][j] = S[j][i] = tot[21 + idx]; }
    // H = L L^T; a pivot <= 0 (not NaN: a zero range propagates) means no estimate
    bool ok = true;
    double id[6]; // 1 / L[j][j]
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dgn = H[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) dgn -= L[j][k] * L[j][k];
        if (dgn <= 0.0) ok = false;
        L[j][j] = sqrt(dgn);
        id[j] = 1.0 / L[j][j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = H[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v * id[j];
        }
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 36; ++i) cov[i] = (i % 7 == 0) ? 3.402823466e38f : 0.f;
        return;
    }
    // H^-1, column by column: L y = e_c, L^T x = y
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double v = (i == cc) ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
            y[i] = v * id[i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double v = y[i];
#pragma unroll
            for (int k = i + 1; k < 6; ++k) v -= L[k][i] * Hi[k][cc];
            Hi[i][cc] = v * id[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) v += Hi[i][k] * S[k][j];
            M[i][j] = v;
        }
    const double s2 = (double)sigma * (double)sigma;
    // the upper triangle, mirrored: Cov is symmetric to the bit
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) v += M[i][k] * Hi[k][j];
            const float f = (float)(s2 * v);
            cov[6 * j + i] = f; cov[6 * i + j] = f;
        }
}

const float* loop_covariance_out(const icpmi_ctx* c) { return reinterpret_cast<const float*>(c->d_cov + ICPMI_COV_NB * ICPMI_COV_NV); }

icpmi_status loop_covariance(icpmi_ctx* c, int64_t n, const LoopCfg& lc, bool sorted)
{
    if (c->d_cov.ensure(c, (size_t)ICPMI_COV_NB * ICPMI_COV_NV + 18) != ICPMI_OK) return ICPMI_ERR_HIP; // (+ 36 floats)
    hipLaunchKernelGGL(cov_pairs_kernel, dim3(ICPMI_COV_NB), dim3(256), 0, c->stream, pair_view(c, lc, sorted), (int)n, lc, c->d_state, c->d_cov);
    hipLaunchKernelGGL(cov_solve_kernel, dim3(1), dim3(256), 0, c->stream, c->d_cov, ICPMI_COV_NB, c->cfg.sensor_std_dev,
                       const_cast<float*>(loop_covariance_out(c)));
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// ---------------------------------------------------------------------------------------------
// Degeneracy-aware point-to-plane solve (solve.h: degen_*; include/icpmi.h: icpmi_get_localizability): the reading's statistics in the
// registration's head, the report behind the loop.  c0 = mean of the centred reading, L = mean |p - c0|: double, per-workgroup partials in
// a fixed order and then the ICPMI_DG_NB partials in a fixed order -- no atomics, two calls give the same bits.  Launched only when the
// chain asks for the option.
// ---------------------------------------------------------------------------------------------
namespace {

// the mean from the per-workgroup sums, the same order wherever it is formed
__device__ __forceinline__ void degen_mean(const double* __restrict__ blk, int64_t n, double* c0)
{
    double s[3] = {0.0, 0.0, 0.0};
    for (int b = 0; b < ICPMI_DG_NB; ++b)
        for (int r = 0; r < 3; ++r) s[r] += blk[ICPMI_DG_PART + 4 * b + r];
    for (int r = 0; r < 3; ++r) c0[r] = s[r] / (double)n;
}

// MODE 0: per-workgroup sums of x, y, z; MODE 1: per-workgroup sum of |p - c0|
template <int MODE>
__global__ __launch_bounds__(256) void degen_stats_kernel(const float4* __restrict__ reading, int64_t n, double* __restrict__ blk)
{
    __shared__ double sh[256];
    double c0[3] = {0.0, 0.0, 0.0};
    if (MODE == 1) degen_mean(blk, n, c0);
    double a[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)ICPMI_DG_NB * 256) {
        const float4 p = reading[i];
        if (MODE == 0) { a[0] += (double)p.x; a[1] += (double)p.y; a[2] += (double)p.z; }
        else {
            const double x = (double)p.x - c0[0], y = (double)p.y - c0[1], z = (double)p.z - c0[2];
            a[0] += sqrt((x * x + y * y) + z * z);
        }
    }
    for (int r = 0; r < (MODE == 0 ? 3 : 1); ++r) {
        const double s = block_tree_sum(a[r], sh);
        if (threadIdx.x == 0) blk[ICPMI_DG_PART + 4 * blockIdx.x + (MODE == 0 ? r : 3)] = s;
    }
}

__global__ __launch_bounds__(64) void degen_stats_final_kernel(int64_t n, double* __restrict__ blk)
{
    if (threadIdx.x != 0) return;
    double c0[3];
    degen_mean(blk, n, c0);
    double s = 0.0;
    for (int b = 0; b < ICPMI_DG_NB; ++b) s += blk[ICPMI_DG_PART + 4 * b + 3];
    const double L = s / (double)n;
    for (int r = 0; r < 3; ++r) blk[ICPMI_DG_C0 + r] = c0[r];
    blk[ICPMI_DG_C0 + 3] = L == 0.0 ? 1.0 : L;
}

// one lane: steps 1 - 4 on the kept sums of the last counted iteration -> icpmi_localizability (pivot in the centred frame: the host adds the mean)
__global__ __launch_bounds__(64) void degen_report_kernel(double* __restrict__ blk, int four_dof, float thr)
{
    if (threadIdx.x != 0) return;
    __shared__ DegenSys S;
    degen_pivot(blk + ICPMI_DG_T, blk + ICPMI_DG_C0, S.c);
    S.L = blk[ICPMI_DG_C0 + 3];
    degen_decompose(blk + ICPMI_DG_SUMS, four_dof, thr, &S);
    icpmi_localizability* out = reinterpret_cast<icpmi_localizability*>(blk + ICPMI_DG_OUT);
    const int n = S.n, o = four_dof ? 2 : 0;
    out->n = n; out->n_degenerate = S.ndeg;
    for (int e = 0; e < 6; ++e) {
        out->degenerate[e] = S.deg[e];
        out->eigval[e] = (e < n && S.W > 0.0) ? S.w[e] / S.W : 0.0;
        for (int i = 0; i < 6; ++i) out->basis[6 * e + i] = 0.0;
        if (e < n) for (int i = 0; i < n; ++i) out->basis[6 * e + o + i] = S.Q[n * e + i];
    }
    for (int r = 0; r < 3; ++r) out->pivot[r] = S.c[r];
    out->lnorm = S.L; out->weight_sum = S.W;
    out->pairs = (long long)(blk[ICPMI_DG_SUMS + 28] + 0.5);
    out->iterations = (int)blk[ICPMI_DG_ITER];
    for (int i = 0; i < 3; ++i) out->reserved[i] = 0;
}

} // namespace

icpmi_status loop_degen_stats(icpmi_ctx* c, int64_t n, const LoopCfg& lc)
{
    if (!lc.degen || n <= 0) return ICPMI_OK;
    hipLaunchKernelGGL(degen_stats_kernel<0>, dim3(ICPMI_DG_NB), dim3(256), 0, c->stream, (const float4*)c->d_reading.get(), n, lc.degen_blk);
    hipLaunchKernelGGL(degen_stats_kernel<1>, dim3(ICPMI_DG_NB), dim3(256), 0, c->stream, (const float4*)c->d_reading.get(), n, lc.degen_blk);
    hipLaunchKernelGGL(degen_stats_final_kernel, dim3(1), dim3(64), 0, c->stream, n, lc.degen_blk);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

icpmi_status loop_degen_report(icpmi_ctx* c, const LoopCfg& lc)
{
    hipLaunchKernelGGL(degen_report_kernel, dim3(1), dim3(64), 0, c->stream, lc.degen_blk, lc.force_4dof, lc.degen_thr);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// head_done: the caller wants the loop state initialised too (enqueue_registration_head); set when the sort's kernels did it.  Centring,
// loop-state initialisation and the clearing of the selection histograms ride in the kernels of the query sort (SortHead) -- the head of a
// registration is 3 graph nodes instead of 8
icpmi_status loop_prepare_reading(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_normals3, bool* head_done)
{
    if (c->d_reading.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    const int blocks = (int)((n + 255) / 256);
    // (the head of a VoxelMatcher registration: nothing on that path reads the tile-sorted copy, so the reading is centred and left in the
    // caller's order -- centre_kernel below, the loop state by enqueue_registration_head)
    const bool no_sort = head_done && voxel_path(c);
    const bool fused = head_done && c->cfg.knn <= 8 && n > 0 && !no_sort;
    if (head_done) *head_done = fused;
    if (blocks && !fused) {
        BatchSrc src; memset(&src, 0, sizeof src); src.p[0] = d_scan;
        hipLaunchKernelGGL(centre_kernel, dim3(blocks), dim3(256), 0, c->stream, src, batch_of_one(n), c->mean[0], c->mean[1], c->mean[2], c->d_reading);
    }
    if (d_normals3) {
        if (c->d_read_normals.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        if (blocks) hipLaunchKernelGGL(pad_normals_kernel, dim3(blocks), dim3(256), 0, c->stream, d_normals3, n, c->d_read_normals);
    }
    HIP_TRY(c, hipGetLastError());
    // tile order of the (centred) reading: wave-local cell coherence for the pyramid NN kernels
    if (fused) {
        SortHead h; memset(&h.raw, 0, sizeof h.raw);
        h.raw.p[0] = d_scan; h.mean[0] = c->mean[0]; h.mean[1] = c->mean[1]; h.mean[2] = c->mean[2];
        h.st = c->d_state; h.seq = c->reg_seq; h.progress = c->d_progress; h.seq_src = c->d_progress + 32;
        h.selhist = c->d_selhist;
        return sort_queries_batch(c, c->d_reading, batch_of_one(n), &h);
    }
    if (c->cfg.knn <= 8 && n > 0 && !no_sort) return sort_queries(c, c->d_reading, n);
    return ICPMI_OK;
}

// The reading as a voxel registration's head prepares it, into buffers of the caller's (voxel.hip: voxel_score_poses): centred in the
// caller's order, the normals padded.  Nothing of the handle's own reading, loop state or captured loop is touched.
icpmi_status loop_centre_pad(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_normals3, float4* d_pts, float4* d_nrm)
{
    const int blocks = (int)((n + 255) / 256);
    if (!blocks) return ICPMI_OK;
    BatchSrc src; memset(&src, 0, sizeof src); src.p[0] = d_scan;
    hipLaunchKernelGGL(centre_kernel, dim3(blocks), dim3(256), 0, c->stream, src, batch_of_one(n), c->mean[0], c->mean[1], c->mean[2], d_pts);
    hipLaunchKernelGGL(pad_normals_kernel, dim3(blocks), dim3(256), 0, c->stream, d_normals3, n, d_nrm);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

static int acc_cap()
{
    static int cap = -1;
    if (cap < 0) {
        cap = 256; // (r4 sweep 256 / 300 / 400 / 600: one 1 024-thread workgroup per CU wins)
        // the limb headroom of the fixed-point accumulators (common.h) is sized for ICPMI_ACC_MAX_ADDS workgroup partials per copy
        if (cap > ICPMI_ACC_MAX_ADDS * ICPMI_ACC_COPIES) cap = ICPMI_ACC_MAX_ADDS * ICPMI_ACC_COPIES;
    }
    return cap;
}

static int acc_blocks(int64_t count, int bt = 256)
{
    const int cap = acc_cap();
    const int64_t nb = (count + bt - 1) / bt;
    return (int)(nb < 1 ? 1 : (nb > cap ? cap : nb));
}

// words of icpmi_ctx::d_defer for a reading of n points: three lists of eight entries per helper workgroup, one flag per query slot
static size_t defer_words(const icpmi_ctx* c, int64_t n) { return (size_t)3 * 8 * (size_t)c->nn_defer_wgs + (size_t)n + 1; }

// everything the loop's launches for chain lc write to: n = points per slice, nscan slices (a single registration: one slice of n points).
// The VarTrimmedDist scratch is reserved here too, so that enqueue_selection cannot fail (such a chain never takes a batch).
icpmi_status ensure_loop_buffers(icpmi_ctx* c, int64_t n, const LoopCfg& lc, int nscan)
{
    const size_t cnt = (size_t)n * lc.k * nscan + 1;
    if (c->d_sidx.ensure(c, cnt) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_d2.ensure(c, cnt) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_hard.ensure(c, (size_t)n * nscan + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (lc.k == 1 && c->d_match_pt.ensure(c, (size_t)n * nscan + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (lc.k == 1 && nscan == 1 && c->nn_defer) { // the k = 1 matcher's defer lists and flags (nn.hip: nn1_wg_kernel); a new block starts zeroed
        bool fresh = false;
        if (c->d_defer.ensure(c, defer_words(c, n), &fresh) != ICPMI_OK) return ICPMI_ERR_HIP;
        if (fresh) HIP_TRY(c, hipMemsetAsync(c->d_defer, 0, c->d_defer.capacity() * sizeof(unsigned), c->stream));
    }
    if (c->d_selhist.ensure(c, (size_t)ICPMI_SELHIST_WORDS * nscan) != ICPMI_OK) return ICPMI_ERR_HIP;
    return selection_reserve(c, lc, n * lc.k);
}

// The pair sums of model PM on the stream.  THE place that resolves the kernel's other three variants: FUSED (slot >= 0: the chain's single
// quantile filter, whose last selection level the kernel scans itself), EXT (a GenericDescriptor / Robust filter or force2D: rare, its own
// instantiation keeps the common kernels as they were) and the workgroup size (acc_threads).
// sorted: the loop state is in query order (NnOutcome::out_sorted; k = 1: with the matched points, see nn1_wg_kernel; k > 1: ids and d2)
template <PairModel PM>
static void launch_accumulate(icpmi_ctx* c, const LoopCfg& lc, int nb, int slot, const BatchArgs& ba, bool sorted)
{
    const PairView v = pair_view(c, lc, sorted); // (match_pt is null for k > 1)
    const int is_med = slot >= 0 && lc.out_type[slot] == ICPMI_OUT_MEDIANDIST;
    const float factor = slot >= 0 ? lc.out_param[slot] : 0.f;
    // k > 1, a model that reads the map's normals: matched point and its normal side by side (map_build.hip: pn_kernel)
    const float4* pnm = (lc.k > 1 && pair_reads_map_normals(PM) && c->has_normals && c->d_map_pn) ? c->d_map_pn.get() : nullptr;
    const auto launch = [&](auto fused, auto ext, auto bt) {
        hipLaunchKernelGGL((accumulate_kernel<PM, fused.value, ext.value, bt.value>), dim3(nb, ba.nscan), dim3(bt.value), 0, c->stream, v.reading, ba, acc_cap(), lc,
                           c->d_state, v.map, v.ref_normals, v.read_normals, v.sidx, v.d2, c->d_selhist, slot, is_med, factor, v.match_pt, v.qindex,
                           v.ref_scalar, pnm);
    };
    const auto sized = [&](auto fused, auto ext) {
        if (acc_threads(lc.k) == 1024) launch(fused, ext, std::integral_constant<int, 1024>{});
        else launch(fused, ext, std::integral_constant<int, 256>{});
    };
    const bool fused = slot >= 0, ext = lc.ext != 0;
    if (fused && ext) sized(std::true_type{}, std::true_type{});
    else if (fused) sized(std::true_type{}, std::false_type{});
    else if (ext) sized(std::false_type{}, std::true_type{});
    else sized(std::false_type{}, std::false_type{});
}

// publish = false: this solve leaves the progress word alone (an iteration inside a fixed-count graph: see loop_run)
static void enqueue_accumulate_solve(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const BatchArgs& ba, const NnOutcome& nn, float* d_Tstep, double* d_sums,
                                     bool publish = true)
{
    const int64_t count = n * lc.k;
    const int nb = acc_blocks(count, acc_threads(lc.k));
    const int slot = fused_filter_slot(lc);
    // (r1: letting the last pair-sum workgroup solve -- ticket + device fences -- measured +3.5 us per
    // iteration against this separate 1-workgroup launch, and dragged the solver's registers and scratch
    // into the pair-sum kernel: removed.)
    switch (lc.pair_model) { // (the solve below reads lc.minimizer: point-to-plane for the last four)
    case PAIR_SYMMETRIC: launch_accumulate<PAIR_SYMMETRIC>(c, lc, nb, slot, ba, nn.out_sorted); break;
    case PAIR_PLANE_TO_PLANE: launch_accumulate<PAIR_PLANE_TO_PLANE>(c, lc, nb, slot, ba, nn.out_sorted); break;
    case PAIR_INTENSITY: launch_accumulate<PAIR_INTENSITY>(c, lc, nb, slot, ba, nn.out_sorted); break;
    case PAIR_POINT_TO_PLANE: launch_accumulate<PAIR_POINT_TO_PLANE>(c, lc, nb, slot, ba, nn.out_sorted); break;
    case PAIR_POINT_TO_POINT: launch_accumulate<PAIR_POINT_TO_POINT>(c, lc, nb, slot, ba, nn.out_sorted); break;
    default: launch_accumulate<PAIR_IDENTITY>(c, lc, nb, slot, ba, nn.out_sorted); break;
    }
    if (lc.degen) // (a single registration: chain_takes_batch keeps such a handle out of the batched loop)
        hipLaunchKernelGGL(solve_kernel<true>, dim3(ba.nscan), dim3(256), 0, c->stream, c->d_state, c->d_selhist, 1, lc, d_Tstep, d_sums,
                           publish ? c->d_progress : (unsigned*)nullptr, ba.nscan == 1 ? c->d_state_mirror : (IcpState*)nullptr);
    else
        hipLaunchKernelGGL(solve_kernel<false>, dim3(ba.nscan), dim3(256), 0, c->stream, c->d_state, c->d_selhist, 1, lc, d_Tstep, d_sums,
                           publish ? c->d_progress : (unsigned*)nullptr, ba.nscan == 1 ? c->d_state_mirror : (IcpState*)nullptr);
}

// the iteration of a VoxelMatcher handle (voxel_path; a single registration): voxel_pairs_kernel fills the point-to-plane slots of the
// accumulators, the solve reads them as it reads plane-to-plane's (lc.plane_eps: the same epsilon)
static void enqueue_voxel_solve(icpmi_ctx* c, int64_t n, const LoopCfg& lc, float* d_Tstep, double* d_sums, bool publish, bool advance = true)
{
    voxel_enqueue_pairs(c, n, acc_blocks(n), lc.plane_eps);
    if (voxel_scheduled(c)) {
        // a schedule: the solve tells the host nothing -- its stop may be a level switch; voxel_advance_kernel behind it
        // decides, and mirrors and publishes in its place.  advance = false: one pass at a fixed level (loop_single_step), no switch to make
        hipLaunchKernelGGL(solve_kernel<false>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, 1, lc, d_Tstep, d_sums, (unsigned*)nullptr,
                           (IcpState*)nullptr);
        if (advance)
            hipLaunchKernelGGL(voxel_advance_kernel, dim3(1), dim3(64), 0, c->stream, c->d_state.get(), c->d_vox_sched.get(), c->vox_levels,
                               publish ? c->d_progress : (unsigned*)nullptr, c->d_state_mirror, c->d_progress + ICPMI_PROGRESS_VOX_WORD);
        return;
    }
    hipLaunchKernelGGL(solve_kernel<false>, dim3(1), dim3(256), 0, c->stream, c->d_state, c->d_selhist, 1, lc, d_Tstep, d_sums,
                       publish ? c->d_progress : (unsigned*)nullptr, c->d_state_mirror);
}

// what every launch of a registration's loop asks of the matcher (ba: its readings; NnRequest::iter is set iteration by iteration).  Built
// once the loop's buffers have their final size.
NnRequest loop_request(icpmi_ctx* c, const LoopCfg& lc, const BatchArgs& ba, const float* d_r2row)
{
    NnRequest req;
    req.hist0 = fused_filter_slot(lc) >= 0 ? c->d_selhist.get() : nullptr;
    req.match_pt = lc.k == 1 ? c->d_match_pt.get() : nullptr;
    req.sorted_k = lc.k > 1;
    req.r2row = d_r2row;
    req.batch = ba;
    // (one reading, and only behind an ensure_loop_buffers that reserved the lists for it: a batch keeps every query in its home workgroup)
    if (lc.k == 1 && ba.nscan <= 1 && c->nn_defer && c->d_defer.get() && c->d_defer.capacity() >= defer_words(c, ba.n[0])) {
        req.defer = c->d_defer.get();
        req.defer_wgs = c->nn_defer_wgs;
    }
    return req;
}

// the chain as the entry points that run ONE pass of it see it: one iteration, no checkers
LoopCfg one_pass_cfg(const LoopCfg& lc)
{
    LoopCfg l1 = lc;
    l1.max_iter = 1; l1.use_diff = 0; l1.use_bound = 0;
    return l1;
}

// nstates fresh loop states outside a registration (no sequence number, no progress word) and their cleared selection histograms;
// d_T0: one pose of 16 floats per state, null = identity
icpmi_status enqueue_fresh_states(icpmi_ctx* c, int nstates, const float* d_T0)
{
    hipLaunchKernelGGL(init_state_kernel, dim3(nstates), dim3(64), 0, c->stream, c->d_state, d_T0, 0u, (unsigned*)nullptr, (const unsigned*)nullptr, 16);
    HIP_TRY(c, hipMemsetAsync(c->d_selhist, 0, (size_t)ICPMI_SELHIST_WORDS * nstates * sizeof(unsigned), c->stream));
    return ICPMI_OK;
}

// the front of an iteration: the matcher's launch under the states' T_iter, then the chain's selections; *nn = what the launch answered.
// matched: recorded between the two (a profiled registration times its matcher)
icpmi_status enqueue_match_select(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const NnRequest& req, NnOutcome* nn, hipEvent_t matched)
{
    const icpmi_status s = nn_launch_k(c, req, c->d_reading, n, c->d_state->T_iter, lc, 1, c->d_sidx, c->d_d2, c->d_state, nn);
    if (s != ICPMI_OK) return s;
    if (matched) HIP_TRY(c, hipEventRecord(matched, c->stream));
    enqueue_selection(c, lc, n * lc.k, req.batch, *nn);
    return ICPMI_OK;
}

// iteration req.iter of the loop: match, select, accumulate, solve
static icpmi_status enqueue_iteration(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const NnRequest& req, NnOutcome* nn, hipEvent_t nn0, hipEvent_t nn1,
                                      bool publish = true)
{
    if (nn0) HIP_TRY(c, hipEventRecord(nn0, c->stream));
    if (voxel_path(c)) { // VoxelMatcher (voxel.hip): no matcher, no selection -- the voxel pair sums, then the solve every chain ends in
        enqueue_voxel_solve(c, n, lc, nullptr, c->d_keep_sums.get(), publish);
        if (nn1) HIP_TRY(c, hipEventRecord(nn1, c->stream));
        HIP_TRY(c, hipGetLastError());
        return ICPMI_OK;
    }
    { const icpmi_status s = enqueue_match_select(c, n, lc, req, nn, nn1); if (s != ICPMI_OK) return s; }
    // (icpmi_debug_keep_sums: the sums of every counted iteration of a SINGLE registration; a batch's solves would all write the one block)
    enqueue_accumulate_solve(c, n, lc, req.batch, *nn, nullptr, req.batch.nscan > 1 ? nullptr : c->d_keep_sums.get(), publish);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// with_dbg = false (the batch path): reserved[] stays as the caller cleared it
static void fill_stats(const IcpState* hs, const LoopCfg& lc, int64_t n, icpmi_stats* stats, bool with_dbg = true)
{
    if (!stats) return;
    stats->iterations = hs->iter;
    stats->stop_reason = hs->stop_reason;
    stats->pairs = hs->pairs;
    const double denom = (double)lc.k * (double)n;
    stats->point_used_ratio = denom > 0 ? (float)hs->pairs / (float)denom : 0.f;
    stats->weighted_point_used_ratio = denom > 0 ? (float)(hs->wsum / denom) : 0.f;
    const int q = quantile_slot(lc);
    stats->trimmed_limit = q >= 0 ? hs->limits[q] : -1.f;
    stats->hard_queries = (int64_t)hs->hard_total;
    stats->sensor_noise_overlap = -1.f; // "not computed" unless loop_run's sensor-noise pass overwrites it
    for (int i = 0; i < 2 && with_dbg; ++i) { stats->reserved[2 * i] = (int32_t)(hs->dbg[i] & 0xffffffffu); stats->reserved[2 * i + 1] = (int32_t)(hs->dbg[i] >> 32); }
}

static void host_mat4_mul(const float* A, const float* B, float* C)
{
    float R[16];
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            float s = A[i] * B[4 * j];
            for (int kk = 1; kk < 4; ++kk) s = fmaf(A[4 * kk + i], B[4 * j + kk], s);
            R[4 * j + i] = s;
        }
    memcpy(C, R, sizeof R);
}

// the registration's result in the caller's frame: T_refIn_refMean * T_iter * T_refMean_dataIn
static void pose_out(const icpmi_ctx* c, const float* T_iter, float* T_out)
{
    float Tm[16], Tmi[16], tmp[16];
    for (int i = 0; i < 16; ++i) Tm[i] = Tmi[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; ++r) { Tm[12 + r] = c->mean[r]; Tmi[12 + r] = -c->mean[r]; }
    host_mat4_mul(T_iter, Tmi, tmp);
    host_mat4_mul(Tm, tmp, T_out);
}

// everything a registration enqueues before its first iteration: centring + tile sort of the reading,
// loop state, selection histograms
static icpmi_status enqueue_registration_head(icpmi_ctx* c, const float4* d_scan, const float* d_normals3, int64_t n, const LoopCfg& lc)
{
    bool head_done = false;
    icpmi_status s = loop_prepare_reading(c, d_scan, n, d_normals3, &head_done);
    if (s != ICPMI_OK) return s;
    if (lc.degen) { s = loop_degen_stats(c, n, lc); if (s != ICPMI_OK) return s; } // (c0, L of the centred reading: once per registration)
    if (head_done) return ICPMI_OK;
    // (the registration's sequence number: loop_run stores it in h_progress[32] before it launches anything)
    hipLaunchKernelGGL(init_state_kernel, dim3(1), dim3(64), 0, c->stream, c->d_state, (const float*)nullptr, c->reg_seq, c->d_progress,
                       (const unsigned*)(c->d_progress + 32));
    HIP_TRY(c, hipMemsetAsync(c->d_selhist, 0, ICPMI_SELHIST_WORDS * sizeof(unsigned), c->stream));
    if (voxel_scheduled(c)) // (every registration starts at level 0 with a clean report)
        hipLaunchKernelGGL(voxel_sched_reset_kernel, dim3(1), dim3(64), 0, c->stream, c->d_state.get(), c->d_vox_sched.get(), 0u);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// Capture what enqueue() puts on the handle's stream (a head and the iterations behind it) into g, replacing what g held; g then serves the
// registrations of signature `sig`.  enqueue(&nn) leaves in nn what the matcher's last launch answered.
template <class Enqueue>
static icpmi_status capture_loop_graph(icpmi_ctx* c, LoopGraph& g, uint64_t sig, Enqueue enqueue)
{
    g.reset();
    hipGraph_t gr = nullptr;
    CaptureGate capture_scope; // (common.h: no device-wide synchronisation of another thread while this one captures)
    HIP_TRY(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    NnOutcome nn;
    const icpmi_status s = enqueue(&nn);
    const hipError_t ce = hipStreamEndCapture(c->stream, &gr);
    if (s != ICPMI_OK) { if (gr) hipGraphDestroy(gr); return s; }
    HIP_TRY(c, ce);
    const hipError_t ie = hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0);
    hipGraphDestroy(gr);
    HIP_TRY(c, ie);
    g.sig = sig; g.uses = 1; g.sorted = nn.out_sorted;
    return ICPMI_OK;
}

// what a graph of loop_run is valid for: the chain (its iteration count, hence the segment length, included), the reading's size, every
// buffer its launches take a pointer to, the grid and the map epoch
static uint64_t loop_sig(const icpmi_ctx* c, const LoopCfg& lc, const NnRequest& req, const float4* d_scan, const float* d_normals3, int64_t n)
{
    uint64_t sig = fnv(&lc, sizeof lc, 1469598103934665603ull);
    const void* ptrs[] = {d_scan, d_normals3, c->d_qkeys, c->d_qtile, c->d_reading, c->d_read_normals, c->d_sidx, c->d_d2, c->d_hard, c->d_state, c->d_match_pt,
                          c->d_qsorted, c->d_qindex, c->d_map_sorted, c->d_normals_sorted, c->d_cell_start, c->d_selhist, req.r2row,
                          c->scratch[0], c->scratch[1], c->scratch[2], c->scratch[3], c->scratch[4], // (VarTrimmedDist passes)
                          req.defer};
    sig = fnv(ptrs, sizeof ptrs, sig);
    sig = fnv(&c->grid, sizeof c->grid, sig);
    sig = fnv(&c->map_epoch, sizeof c->map_epoch, sig);
    if (voxel_path(c)) { // (sizes and tables are arguments of the voxel pair kernels alone, not part of the LoopCfg: the level count, every level's
                         // size, table generation and table address, and the block the descriptors sit in)
        const void* sched = c->d_vox_sched.get();
        sig = voxel_sched_sig(c, sig);
        sig = fnv(&sched, sizeof sched, sig);
    }
    return fnv(&n, sizeof n, sig);
}

// r5: a mapper rebuilds its map behind every scan (Map::updateLocalPointCloud -> icp.setMap), and every rebuild drops the graphs: capture +
// instantiate + destroy per scan cost more than they saved (chain bench: register 0.58 -> 0.455 ms, update 1.53 -> 1.45 ms with no graph at
// all).  After two sets of a kind in a row that served one registration each (`wasted`, counted by drop_loop_graphs) the handle runs that
// kind eagerly, until the same signature comes back twice (localisation against a fixed map, the benchmark's repeats): then a graph pays again.
static bool go_eager(icpmi_ctx* c, int* wasted, bool cached, uint64_t sig)
{
    if (cached || *wasted < 2) return false;
    if (c->eager_sig == sig) { *wasted = 0; return false; }
    c->eager_sig = sig;
    return true;
}

icpmi_status loop_run(icpmi_ctx* c, const float4* d_scan, const float* d_normals3, int64_t n, const LoopCfg& lc_in, const float* d_r2row,
                      bool fixed, float T_out[16], icpmi_stats* stats)
{
    LoopCfg lc = lc_in;
    c->last_match_n = 0; c->cov_ready = false; c->cov_kept = false; c->degen_ready = false;
    // all allocations up front: none may happen while the stream is capturing
    if (ensure_loop_buffers(c, n, lc) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_reading.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (d_normals3 && c->d_read_normals.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    const bool voxel = voxel_path(c);
    // a schedule: lc.max_iter bounds a LEVEL (the solve's Counter starts afresh at each), the loop as the host enqueues it
    // is bounded by levels x that count; the progress word counts the iterations of all levels
    const bool sched = voxel_scheduled(c);
    const int total_iter = sched ? (lc.max_iter < 0xfff ? lc.max_iter * c->vox_levels : lc.max_iter) : lc.max_iter;
    // (the report words of the host page are left alone here: dead iterations of the handle's previous registration may still be writing
    // their own final values; this registration's advance overwrites them in stream order, in front of its "done" word)
    if (sched) for (int i = 0; i < 1 + 3 * ICPMI_MAX_VOXEL_LEVELS; ++i) c->vox_report[i] = 0;
    if (voxel) { c->qsorted_n = -1; c->qsorted_src = nullptr; } // (d_reading gets new contents and no sorted copy: a stale one must not be searched in its place)
    else if (c->cfg.knn <= 8 && sort_queries_reserve(c, n) != ICPMI_OK) return ICPMI_ERR_HIP;
    NnRequest req = loop_request(c, lc, batch_of_one(n), d_r2row);
    NnOutcome last; // what the last eagerly enqueued iteration's launch answered (a graph keeps its own: LoopGraph::sorted)

    const bool profile = c->cfg.profile != 0;
    bool graph = c->cfg.use_graph != 0 && fixed && !profile;
    float nn_ms_sum = 0.f; int nn_cnt = 0;
    c->reg_seq = (c->reg_seq + 1) & 0x7ffffu;
    __atomic_store_n(c->h_progress + 32, c->reg_seq, __ATOMIC_RELEASE);
    // r5 (fast finish, see the end of this function): the finished state reaches the host by itself and carries the device clocks of its
    // start and stop -- no event pair, no copy, no drain
    const bool fast_ok = !profile && c->d_state_mirror && total_iter < 0xfff;
    if (!fast_ok) HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    // A checked loop (Counter + Differential / Bound: what Mapper::processInput runs) as SEGMENT graphs (r3):
    // head + the first S iterations are one graph, S further iterations another; a segment is launched when the progress word
    // says the loop is still running and within S / 2 iterations of the end of what is enqueued.  Iterations past the stop are
    // early-exit kernels (every kernel of the loop returns on st->done): at most S - 1 of them, against eager launches -- and
    // their wider kernel-to-kernel gaps -- for every real iteration.
    bool segmented = !graph && !profile && c->cfg.use_graph != 0 && (lc.use_diff || lc.use_bound) && total_iter < 0xfff && lc.max_iter > 1;
    const int S = std::min(4, lc.max_iter);
    LoopGraphs& gs = c->graphs;
    const uint64_t sig = (graph || segmented) ? loop_sig(c, lc, req, d_scan, d_normals3, n) : 0;
    const bool cached = segmented ? gs.seg[0].holds(sig) && gs.seg[1].holds(sig) : gs.fixed.holds(sig);
    if (segmented && go_eager(c, &c->seg_wasted, cached, sig)) segmented = false;
    // (the same rule for the one-graph registration of a Counter-only chain: the shipped configuration, examples/config.yaml:54-57)
    if (graph && go_eager(c, &c->graph_wasted, cached, sig)) graph = false;
    // head (when asked) + `count` iterations from iteration `first` on, in the order every path enqueues them
    // last_word_only: only the last of the `count` solves publishes the progress word
    auto enqueue_loop = [&](bool with_head, int first, int count, NnOutcome* nn, bool last_word_only = false) {
        icpmi_status s = with_head ? enqueue_registration_head(c, d_scan, d_normals3, n, lc) : ICPMI_OK;
        for (int it = 0; it < count && s == ICPMI_OK; ++it) {
            req.iter = first + it;
            s = enqueue_iteration(c, n, lc, req, nn, nullptr, nullptr, !last_word_only || it + 1 == count);
        }
        return s;
    };
    if (!graph && !segmented) {
        icpmi_status s = enqueue_registration_head(c, d_scan, d_normals3, n, lc);
        if (s != ICPMI_OK) return s;
    }
    if (segmented) {
        ++gs.seg[0].uses;
        if (!cached) {
            for (LoopGraph& hd : gs.heads) hd.reset(); // (captured the same pointers)
            // (later segments: every iteration is seeded and past the wide first launches -- one graph serves them all)
            for (int g = 0; g < 2; ++g) {
                const icpmi_status s = capture_loop_graph(c, gs.seg[g], sig, [&](NnOutcome* nn) { return enqueue_loop(g == 0, g == 0 ? 0 : S, S, nn); });
                if (s != ICPMI_OK) return s;
            }
        }
        // r5: the head graph's length follows the handle's previous checked registration.  A mapper registers scan after scan against almost
        // the same map from almost the same prior: the loop stops after the same few iterations every time (6 in the benchmark scene), and
        // head + 4 followed by a segment of 4 ran two dead iterations (eight early-exit launches, ~24 us of a 0.37 ms registration) behind the
        // stop.  With a head of exactly the previous count the host waits for that head to finish (no look-ahead: the prediction says the loop
        // is over) and goes on with ordinary segments only if it is not.
        LoopGraph* head = &gs.seg[0];
        const int L = c->seg_prev_iters;
        if (L >= 2 && L != S && L <= 24 && L < total_iter) {
            head = nullptr;
            for (LoopGraph& hd : gs.heads) if (hd.exec && hd.len == L) head = &hd;
            if (!head) {
                head = &gs.heads[0];
                for (LoopGraph& hd : gs.heads) if (!hd.exec) { head = &hd; break; } else if (hd.used < head->used) head = &hd;
                const icpmi_status s = capture_loop_graph(c, *head, sig, [&](NnOutcome* nn) { return enqueue_loop(true, 0, L, nn); });
                if (s != ICPMI_OK) return s;
                head->len = L;
            }
            head->used = ++gs.clock;
        }
        const int head_len = head == &gs.seg[0] ? S : L;
        HIP_TRY(c, hipGraphLaunch(head->exec, c->stream));
        if (c->cfg.knn <= 8 && !voxel) { c->qsorted_n = n; c->qsorted_src = c->d_reading; } // what the replayed head leaves in d_qsorted
        int launched = head_len;
        while (launched < total_iter) {
            // (behind a predicted head: no look-ahead -- the next segment goes out only once the head has run and the loop is still going)
            const int lead = (launched == head_len && head_len != S) ? 0 : (S > 1 ? S / 2 : 1);
            unsigned v = 0; bool idle = false;
            HIP_TRY(c, spin_on_host(c->stream, 256, c->h_progress, 1, &v, [&](const unsigned* w) {
                const ProgressWord p = decode_progress(*w, c->reg_seq);
                return p.mine && (p.done || p.iter + lead >= launched);
            }, &idle));
            const ProgressWord p = decode_progress(v, c->reg_seq);
            if (idle ? !p.mine || p.done || p.iter < launched : p.done) break; // (idle: everything enqueued has run, the word is final)
            HIP_TRY(c, hipGraphLaunch(gs.seg[1].exec, c->stream));
            launched += S;
        }
    } else if (graph) {
        // the whole registration -- head and all iterations -- is one graph, replayed while the scan
        // buffer, the map and the chain stay the same
        ++gs.fixed.uses;
        if (!cached) {
            // Nobody reads the progress word of a fixed-count graph before its last solve: the host waits for "done", which only that solve
            // (or, behind an error, its early-exit path) can report with the loop's last kernel behind it.  The solves in front of it skip
            // the word and with it the system-scope release that goes with the store.
            const icpmi_status s = capture_loop_graph(c, gs.fixed, sig, [&](NnOutcome* nn) { return enqueue_loop(true, 0, total_iter, nn, true); });
            if (s != ICPMI_OK) return s;
        }
        HIP_TRY(c, hipGraphLaunch(gs.fixed.exec, c->stream));
        if (c->cfg.knn <= 8 && !voxel) { c->qsorted_n = n; c->qsorted_src = c->d_reading; } // what the replayed head leaves in d_qsorted
    } else {
        const int check_every = (lc.use_diff || lc.use_bound) ? 4 : total_iter;
        if (profile && c->nn_events.size() < (size_t)2 * total_iter) {
            while (c->nn_events.size() < (size_t)2 * total_iter) {
                hipEvent_t e; HIP_TRY(c, hipEventCreate(&e)); c->nn_events.push_back(e);
            }
        }
        // A loop of data-dependent length (Differential / Bound) is enqueued a bounded number of iterations ahead of the
        // progress word the solve kernel publishes in host-mapped memory: the stream never drains for a read-back (r1:
        // a hipMemcpy + hipStreamSynchronize every 4 iterations, ~25 us of idle GPU each), and at most `ahead` iterations
        // run as early-exit kernels after the loop has stopped.
        constexpr int ahead = 2;
        const bool poll = !profile && (lc.use_diff || lc.use_bound) && total_iter < 0xfff;
        int launched = 0;
        bool stopped = false;
        for (int it = 0; it < total_iter && !stopped; ++it) {
            hipEvent_t e0 = profile ? c->nn_events[2 * it] : nullptr, e1 = profile ? c->nn_events[2 * it + 1] : nullptr;
            req.iter = it;
            icpmi_status s = enqueue_iteration(c, n, lc, req, &last, e0, e1);
            if (s != ICPMI_OK) return s;
            ++launched;
            if (it + 1 >= total_iter) break;
            if (poll) {
                // go on as soon as the GPU has finished all but `ahead` of the iterations enqueued so far; an idle stream leaves the word
                // final (a kernel that stops the loop without passing through the solve kernel cannot leave the host waiting)
                unsigned v = 0; bool idle = false;
                HIP_TRY(c, spin_on_host(c->stream, 256, c->h_progress, 1, &v, [&](const unsigned* w) {
                    const ProgressWord p = decode_progress(*w, c->reg_seq);
                    return p.mine && (p.done || p.iter + ahead > it);
                }, &idle));
                const ProgressWord p = decode_progress(v, c->reg_seq);
                stopped = idle ? !p.mine || p.done || p.iter <= it : p.done;
            } else if ((it + 1) % check_every == 0) {
                const IcpState* sd = c->d_state;
                HIP_TRY(c, hipMemcpyAsync(&c->h_state->done, &sd->done, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                if (c->h_state->done) break;
            }
        }
        if (profile) {
            // back-to-back event pair: what two records cost with nothing in between (subtracted below)
            if (c->nn_events.size() < (size_t)2 * total_iter + 2) {
                while (c->nn_events.size() < (size_t)2 * total_iter + 2) { hipEvent_t e; HIP_TRY(c, hipEventCreate(&e)); c->nn_events.push_back(e); }
            }
            HIP_TRY(c, hipEventRecord(c->nn_events[2 * total_iter], c->stream));
            HIP_TRY(c, hipEventRecord(c->nn_events[2 * total_iter + 1], c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            HIP_TRY(c, hipMemcpy(c->h_state, c->d_state, sizeof(IcpState), hipMemcpyDeviceToHost));
            const int iters_done = c->h_state->iter < launched ? c->h_state->iter : launched;
            for (int it = 0; it < iters_done; ++it) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, c->nn_events[2 * it], c->nn_events[2 * it + 1]) == hipSuccess) { nn_ms_sum += ms; ++nn_cnt; }
            }
            float gap = 0.f;
            if (hipEventElapsedTime(&gap, c->nn_events[2 * total_iter], c->nn_events[2 * total_iter + 1]) == hipSuccess && nn_cnt) {
                nn_ms_sum -= gap * nn_cnt;
                if (nn_ms_sum < 0.f) nn_ms_sum = 0.f;
            }
        }
    }
    // r5: the final state is already in c->h_state when the progress word says "done" (solve_kernel: mirror_state), with the device clocks
    // of the head's first kernel and of the solve that stopped the loop in it.  Returning on that word instead of behind an event or a
    // drained stream takes the end-of-graph release and the completion signal (21 - 26 us between the flag and the drained stream,
    // -DICPMI_TAIL_DIAG) off the caller's clock: the next registration is enqueued while they happen.  Whatever this registration still has
    // in the stream (dead iterations behind a stop) touches the handle's own buffers only and stays in stream order with everything the
    // handle enqueues next.  The copy + drain below remains for loops that end without the flag (no Counter in the chain and the host's
    // bound reached, a stream in an error state), for the profiling loop and for ICPMI_FAST_FINISH=0.
    bool have_state = false;
    if (fast_ok) {
        auto finished = [&](const unsigned* w) { const ProgressWord p = decode_progress(*w, c->reg_seq); return p.mine && p.done; };
        unsigned v = 0;
        HIP_TRY(c, spin_on_host(c->stream, 256, c->h_progress, 1, &v, finished)); // (an idle stream: the word is final)
        have_state = finished(&v);
        if (have_state) {
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            const volatile IcpState* hv = c->h_state;
            have_state = hv->done != 0 && hv->seq == c->reg_seq; // (belt and braces: the block belongs to THIS registration)
        }
    } else HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    if (!have_state) {
        HIP_TRY(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }

    fill_stats(c->h_state, lc, n, stats);
    if (sched) { // (final: the advance wrote it in front of the "done" word, or the stream has drained)
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        for (int i = 0; i < 1 + 3 * ICPMI_MAX_VOXEL_LEVELS; ++i) c->vox_report[i] = (int32_t)__atomic_load_n(c->h_progress + ICPMI_PROGRESS_VOX_WORD + i, __ATOMIC_RELAXED);
        if (!c->h_state->done) { // (the host's bound ended a loop no checker stopped: the stream has drained, the report is still on the device)
            c->vox_report[0] = (int32_t)(c->h_state->vox_level & (ICPMI_MAX_VOXEL_LEVELS - 1)) + 1;
            HIP_TRY(c, hipMemcpy(c->vox_report + 1, c->d_vox_sched.get() + ICPMI_VS_ITERS, 3 * ICPMI_MAX_VOXEL_LEVELS * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
    }
    if (segmented) { // what the next checked registration's head graph is cut to (the larger of the last two counts: one dead iteration costs
                     // less than a head that ends one iteration early and a segment behind it)
        const int it_now = c->h_state->error ? 0 : c->h_state->iter;
        c->seg_prev_iters = it_now > c->seg_last_iters ? it_now : c->seg_last_iters;
        c->seg_last_iters = it_now;
    }
    if (stats) {
        float ms = 0.f;
        if (fast_ok) { // device clocks, 100 MHz: head's first kernel -> the solve that stopped the loop (0 when no solve stopped it)
            const unsigned long long t0 = c->h_state->t_start, t1 = c->h_state->t_done;
            stats->loop_ms = (t1 > t0) ? (float)((double)(t1 - t0) * 1e-5) : 0.f;
        } else if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) stats->loop_ms = ms;
        if (profile) { stats->nn_ms_avg = nn_cnt ? nn_ms_sum / nn_cnt : 0.f; stats->nn_launches = nn_cnt; }
        else { // r6: device clocks (100 MHz) from the NN kernel's first workgroup to the first workgroup of the kernel behind it, summed by the loop itself
            const unsigned cnt = c->h_state->nn_count;
            stats->nn_ms_avg = cnt ? (float)((double)c->h_state->t_nn_sum * 1e-5 / (double)cnt) : 0.f;
            stats->nn_launches = (int32_t)cnt;
        }
        stats->sensor_noise_overlap = -1.f;
    }
    // the last counted iteration's matches stay in the loop's buffers (dead iterations behind the stop early-exit before they write)
    const bool sorted_state = graph ? c->graphs.fixed.sorted : (segmented ? c->graphs.seg[1].sorted : last.out_sorted);
    // (a VoxelMatcher loop leaves no matches behind: icpmi_debug_last_matches and the passes over the last pairs have nothing to read)
    if (!c->h_state->error && c->h_state->iter > 0 && !voxel) { c->last_match_n = n; c->last_match_k = lc.k; c->last_match_sorted = sorted_state; }
    if (lc.sensor_noise && stats && !c->h_state->error && c->h_state->iter > 0) {
        // ErrorMinimizer::getOverlap() with sensor noise: one pass over the last iteration's pairs, still in the loop's buffers
        const icpmi_status os = loop_sensor_noise_overlap(c, n, lc, sorted_state, &stats->sensor_noise_overlap);
        if (os != ICPMI_OK) return os;
    }
    if (c->cfg.covariance && !c->h_state->error && c->h_state->iter > 0) {
        // PointToPlaneWithCovErrorMinimizer: two launches over the same pairs; icpmi_get_covariance reads the result
        const icpmi_status cs = loop_covariance(c, n, lc, sorted_state);
        if (cs != ICPMI_OK) return cs;
        c->cov_ready = true;
    }
    if (lc.degen && !c->h_state->error && c->h_state->iter > 0) {
        // icpmi_get_localizability: one launch on what the last counted iteration's solve kept in the side block
        const icpmi_status ds = loop_degen_report(c, lc);
        if (ds != ICPMI_OK) return ds;
        c->degen_ready = true;
    }
    const IcpState* hs = c->h_state;
    if (hs->error) {
        switch (hs->error) {
            case ICPMI_ERR_NO_POINT_TO_MINIMIZE: c->last_error = "ConvergenceError: ErrorMinimizer: no point to minimize"; break;
            case ICPMI_ERR_NO_OUTLIER_TO_FILTER: c->last_error = "ConvergenceError: no outlier to filter"; break;
            case ICPMI_ERR_BOUND: c->last_error = "ConvergenceError: transformation exceeds BoundTransformationChecker limits"; break;
            case ICPMI_ERR_NAN: c->last_error = "ConvergenceError: transformation is not a number"; break;
            default: c->last_error = "device-side error"; break;
        }
        return (icpmi_status)hs->error;
    }
    pose_out(c, hs->T_iter, T_out);
    return ICPMI_OK;
}

// ---------------------------------------------------------------------------------------------
// Batched registration: B readings against the same map, every kernel of the loop launched once per iteration with
// blockIdx.y = reading (NN: B x N queries in one launch; pair sums: B x 256 workgroups; solve: B workgroups).  A single
// registration is latency-bound (~2.4 wave lifetimes of the NN kernel plus four kernel boundaries per
// iteration leave most of the chip idle); B readings share those fixed costs.  Every reading keeps its own IcpState,
// selection histograms and partials, stops on its own checkers (its kernels early-exit on its `done`), and -- the
// kernels being the ones a single registration runs -- ends on the same bits as when registered alone.
// ---------------------------------------------------------------------------------------------
static void batch_result(icpmi_ctx* c, const LoopCfg& lc, const IcpState* hs, int64_t n, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    fill_stats(hs, lc, n, stats, false); // (the batch path never runs the sensor-noise pass)
    if (status) *status = (icpmi_status)hs->error;
    if (hs->error) for (int i = 0; i < 16; ++i) T_out[i] = (i % 5 == 0) ? 1.f : 0.f;
    else pose_out(c, hs->T_iter, T_out);
}

icpmi_status loop_run_batch(icpmi_ctx* c, int B, const float* const* d_scans4, const int64_t* nn, const LoopCfg& lc, bool fixed, float* T_out,
                            icpmi_stats* stats, icpmi_status* status)
{
    c->last_match_n = 0; c->cov_kept = false; c->degen_ready = false; // (icpmi_debug_last_matches serves single registrations only)
    int64_t nmax = 0;
    for (int b = 0; b < B; ++b) nmax = nn[b] > nmax ? nn[b] : nmax;
    const int64_t NS = (nmax + 63) / 64 * 64; // slice stride of the per-query arrays
    BatchArgs ba; memset(&ba, 0, sizeof ba);
    BatchSrc src; memset(&src, 0, sizeof src);
    ba.nscan = B; ba.qstride = (int)NS;
    for (int b = 0; b < B; ++b) { ba.n[b] = (int)nn[b]; src.p[b] = (const float4*)d_scans4[b]; }
    // all allocations up front: none may happen while the stream is capturing
    if (ensure_loop_buffers(c, NS, lc, B) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_reading.ensure(c, (size_t)NS * B + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (sort_queries_reserve(c, NS, B) != ICPMI_OK) return ICPMI_ERR_HIP;
    struct Scope { icpmi_ctx* c; ~Scope() { c->qsorted_n = -1; c->qsorted_src = nullptr; } } scope{c};
    NnRequest req = loop_request(c, lc, ba, nullptr); // (no var-dist row: such a chain registers its readings one by one)
    NnOutcome last; // (of the eager iterations; nothing behind the loop reads a batch's matches)

    // centring, loop states and selection histograms ride in the kernels of the query sort (no reading of a batch is empty: api.hip sends
    // such a batch through the one-by-one route)
    auto head = [&]() -> icpmi_status {
        c->reg_seq = (c->reg_seq + 1) & 0x7ffffu;
        SortHead h; h.raw = src; h.mean[0] = c->mean[0]; h.mean[1] = c->mean[1]; h.mean[2] = c->mean[2];
        h.st = c->d_state; h.seq = c->reg_seq; h.progress = c->d_progress; h.seq_src = nullptr; h.selhist = c->d_selhist;
        return sort_queries_batch(c, c->d_reading, ba, &h);
    };

    const bool graph = c->cfg.use_graph != 0 && fixed && c->cfg.profile == 0;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    if (graph) {
        uint64_t sig = 1469598103934665603ull;
        sig = fnv(&lc, sizeof lc, sig);
        sig = fnv(&ba, sizeof ba, sig);
        sig = fnv(&src, sizeof src, sig);
        const void* ptrs[] = {c->d_qkeys, c->d_qtile, c->d_reading, c->d_sidx, c->d_d2, c->d_hard, c->d_state, c->d_match_pt,
                              c->d_qsorted, c->d_qindex, c->d_map_sorted, c->d_normals_sorted, c->d_cell_start, c->d_selhist};
        sig = fnv(ptrs, sizeof ptrs, sig);
        sig = fnv(&c->grid, sizeof c->grid, sig);
        if (!c->graphs.batch.holds(sig)) {
            const icpmi_status s = capture_loop_graph(c, c->graphs.batch, sig, [&](NnOutcome* nn) {
                icpmi_status s = head();
                for (int it = 0; it < lc.max_iter && s == ICPMI_OK; ++it) { req.iter = it; s = enqueue_iteration(c, nmax, lc, req, nn, nullptr, nullptr); }
                return s;
            });
            if (s != ICPMI_OK) return s;
        }
        HIP_TRY(c, hipGraphLaunch(c->graphs.batch.exec, c->stream));
    } else {
        icpmi_status s = head();
        if (s != ICPMI_OK) return s;
        constexpr int ahead = 2;
        const bool poll = (lc.use_diff || lc.use_bound) && lc.max_iter < 0xfff;
        bool stopped = false;
        for (int it = 0; it < lc.max_iter && !stopped; ++it) {
            req.iter = it;
            s = enqueue_iteration(c, nmax, lc, req, &last, nullptr, nullptr);
            if (s != ICPMI_OK) return s;
            if (it + 1 >= lc.max_iter || !poll) continue;
            // as loop_run: stay `ahead` iterations in front of the slowest reading still running; stop when all have stopped, or when the
            // stream is idle (everything enqueued has run) and no reading still iterates
            unsigned v[ICPMI_MAX_BATCH]; bool idle = false, all_done = true;
            HIP_TRY(c, spin_on_host(c->stream, 256, c->h_progress, B, v, [&](const unsigned* w) {
                bool may_go = true;
                all_done = true;
                for (int b = 0; b < B; ++b) {
                    const ProgressWord p = decode_progress(w[b], c->reg_seq);
                    all_done &= p.mine && p.done;
                    may_go &= p.mine && (p.done || p.iter + ahead > it);
                }
                return all_done || may_go;
            }, &idle));
            stopped = all_done || idle;
            for (int b = 0; b < B && idle; ++b) {
                const ProgressWord p = decode_progress(v[b], c->reg_seq);
                if (p.mine && !p.done && p.iter > it) stopped = false;
            }
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState) * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    icpmi_status sb[ICPMI_MAX_BATCH];
    for (int b = 0; b < B; ++b) {
        batch_result(c, lc, c->h_state + b, nn[b], T_out + 16 * b, stats ? stats + b : nullptr, &sb[b]);
        if (stats) stats[b].loop_ms = ms;
    }
    return fold_status(c, status, sb, B, "register_batch: a reading ended with a convergence error (see the per-reading status)");
}

// ---------------------------------------------------------------------------------------------
// A batch on the voxel path: B readings, each with its own normals, through one loop.  Per iteration two launches (three
// with a schedule) for all members: voxel_pairs_batch_kernel (blockIdx.y = member), the solve every chain ends in (blockIdx.x = member,
// unchanged), voxel_advance_batch_kernel (one wave per member).  A member keeps its own state, accumulators, level and report, stops on its
// own checkers and switches level on its own; its pair sums are added in the order it has alone: it ends on the bits loop_run gives it.
// Tables and the batch block are current (api.hip: voxel_ensure_table, voxel_ensure_batch_block); no member is empty.  Enqueued eagerly,
// `ahead` iterations in front of the slowest member still running; no captured graph (the results are the same bits either way).
// ---------------------------------------------------------------------------------------------
icpmi_status loop_run_voxel_batch(icpmi_ctx* c, int B, const float* const* d_scans4, const int64_t* nn, const float* const* d_normals3,
                                  const LoopCfg& lc, float* T_out, icpmi_stats* stats, icpmi_status* status)
{
    c->last_match_n = 0; c->cov_ready = false; c->cov_kept = false; c->degen_ready = false;
    int64_t nmax = 0;
    for (int b = 0; b < B; ++b) nmax = nn[b] > nmax ? nn[b] : nmax;
    const int64_t NS = (nmax + 63) / 64 * 64; // slice stride of the centred readings and of the padded normals
    BatchArgs ba; memset(&ba, 0, sizeof ba);
    BatchSrc src; memset(&src, 0, sizeof src);
    ba.nscan = B; ba.qstride = (int)NS;
    for (int b = 0; b < B; ++b) { ba.n[b] = (int)nn[b]; src.p[b] = (const float4*)d_scans4[b]; }
    // all allocations up front
    if (c->d_reading.ensure(c, (size_t)NS * B + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_read_normals.ensure(c, (size_t)NS * B + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_selhist.ensure(c, (size_t)ICPMI_SELHIST_WORDS * B) != ICPMI_OK) return ICPMI_ERR_HIP;
    c->qsorted_n = -1; c->qsorted_src = nullptr; // (d_reading gets new contents and no sorted copy, as in a single voxel loop)
    const bool sched = voxel_scheduled(c);
    const int total_iter = sched ? (lc.max_iter < 0xfff ? lc.max_iter * c->vox_levels : lc.max_iter) : lc.max_iter; // (loop_run's bound)
    unsigned* d_blocks = c->d_vox_batch.get();

    c->reg_seq = (c->reg_seq + 1) & 0x7ffffu;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    // head: centred readings and padded normals into the members' slices, B fresh states and accumulators, level 0 and clean reports.
    // No tile sort: nothing on this path reads it
    hipLaunchKernelGGL(centre_kernel, dim3((int)((nmax + 255) / 256), B), dim3(256), 0, c->stream, src, ba, c->mean[0], c->mean[1], c->mean[2], c->d_reading);
    for (int b = 0; b < B; ++b)
        hipLaunchKernelGGL(pad_normals_kernel, dim3((int)((nn[b] + 255) / 256)), dim3(256), 0, c->stream, d_normals3[b], nn[b],
                           c->d_read_normals.get() + (size_t)b * NS);
    hipLaunchKernelGGL(init_state_kernel, dim3(B), dim3(64), 0, c->stream, c->d_state, (const float*)nullptr, c->reg_seq, c->d_progress,
                       (const unsigned*)nullptr, 0);
    HIP_TRY(c, hipMemsetAsync(c->d_selhist, 0, (size_t)ICPMI_SELHIST_WORDS * B * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(voxel_sched_reset_batch_kernel, dim3(B), dim3(64), 0, c->stream, c->d_state.get(), d_blocks);
    HIP_TRY(c, hipGetLastError());

    const int nb = acc_blocks(nmax);
    constexpr int ahead = 2;
    const bool poll = (lc.use_diff || lc.use_bound) && total_iter < 0xfff;
    bool stopped = false;
    for (int it = 0; it < total_iter && !stopped; ++it) {
        voxel_enqueue_pairs_batch(c, ba, nb, acc_cap(), lc.plane_eps);
        // (with a schedule the solve tells the host nothing -- its stop may be a level switch: the advance behind it publishes)
        hipLaunchKernelGGL(solve_kernel<false>, dim3(B), dim3(256), 0, c->stream, c->d_state, c->d_selhist, 1, lc, (float*)nullptr, (double*)nullptr,
                           sched ? (unsigned*)nullptr : c->d_progress, (IcpState*)nullptr);
        if (sched)
            hipLaunchKernelGGL(voxel_advance_batch_kernel, dim3(B), dim3(64), 0, c->stream, c->d_state.get(), d_blocks, c->vox_levels, c->d_progress);
        HIP_TRY(c, hipGetLastError());
        if (it + 1 >= total_iter || !poll) continue;
        // as loop_run_batch: stay `ahead` iterations in front of the slowest member still running; stop when all have stopped, or when the
        // stream is idle and no member still iterates
        unsigned v[ICPMI_MAX_BATCH]; bool idle = false, all_done = true;
        HIP_TRY(c, spin_on_host(c->stream, 256, c->h_progress, B, v, [&](const unsigned* w) {
            bool may_go = true;
            all_done = true;
            for (int b = 0; b < B; ++b) {
                const ProgressWord p = decode_progress(w[b], c->reg_seq);
                all_done &= p.mine && p.done;
                may_go &= p.mine && (p.done || p.iter + ahead > it);
            }
            return all_done || may_go;
        }, &idle));
        stopped = all_done || idle;
        for (int b = 0; b < B && idle; ++b) {
            const ProgressWord p = decode_progress(v[b], c->reg_seq);
            if (p.mine && !p.done && p.iter > it) stopped = false;
        }
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    unsigned rep[ICPMI_VS_WORDS * ICPMI_MAX_BATCH];
    HIP_TRY(c, hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState) * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rep, d_blocks + ICPMI_VS_WORDS, sizeof(unsigned) * ICPMI_VS_WORDS * B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    icpmi_status sb[ICPMI_MAX_BATCH];
    for (int b = 0; b < B; ++b) {
        const IcpState* hs = c->h_state + b;
        fill_stats(hs, lc, nn[b], stats ? stats + b : nullptr); // (reserved[] as the single call fills it)
        sb[b] = (icpmi_status)hs->error;
        if (hs->error) for (int i = 0; i < 16; ++i) T_out[16 * b + i] = (i % 5 == 0) ? 1.f : 0.f;
        else pose_out(c, hs->T_iter, T_out + 16 * b);
        if (stats) { stats[b].loop_ms = ms; stats[b].nn_ms_avg = 0.f; stats[b].nn_launches = 0; }
        int32_t* r = c->vox_batch_report[b];
        for (int i = 0; i < 1 + 3 * ICPMI_MAX_VOXEL_LEVELS; ++i) r[i] = 0;
        if (sched) { // (what loop_run leaves in vox_report: the levels entered, then iterations, first and last pair counts per level)
            r[0] = (int32_t)(hs->vox_level & (ICPMI_MAX_VOXEL_LEVELS - 1)) + 1;
            for (int i = 0; i < 3 * ICPMI_MAX_VOXEL_LEVELS; ++i) r[1 + i] = (int32_t)rep[(size_t)b * ICPMI_VS_WORDS + ICPMI_VS_ITERS + i];
        }
    }
    return fold_status(c, status, sb, B, "voxel_register_batch: a reading ended with a convergence error (see the per-reading status)");
}

icpmi_status loop_single_step(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const float* T_iter_host, float T_step[16],
                              double sums[32], icpmi_stats* stats)
{
    if (ensure_loop_buffers(c, n, lc) != ICPMI_OK) return ICPMI_ERR_HIP;
    DevBuf<float> d_Tstep; // [0,16): T_step out, [16,32): T_iter in
    DevBuf<double> d_sums;
    HIP_TRY(c, d_Tstep.alloc(32));
    HIP_TRY(c, d_sums.alloc(ICPMI_NV));
    float* d_T0 = d_Tstep.get() + 16;
    if (T_iter_host) HIP_TRY(c, hipMemcpyAsync(d_T0, T_iter_host, 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    { const icpmi_status is = enqueue_fresh_states(c, 1, T_iter_host ? d_T0 : nullptr); if (is != ICPMI_OK) return is; }
    HIP_TRY(c, hipMemsetAsync(d_Tstep, 0, 16 * sizeof(float), c->stream));
    const LoopCfg l1 = one_pass_cfg(lc);
    c->degen_ready = false;
    { const icpmi_status ds = loop_degen_stats(c, n, l1); if (ds != ICPMI_OK) return ds; } // (the reading is in d_reading, centred by the caller)
    NnRequest req; // (one unseeded launch that answers in the caller's order)
    req.hist0 = fused_filter_slot(l1) >= 0 ? c->d_selhist.get() : nullptr;
    req.batch = batch_of_one(n);
    NnOutcome nn;
    const bool voxel = voxel_path(c); // (the table is current: api.hip built it before the reading went up)
    const icpmi_status s = voxel ? ICPMI_OK : enqueue_match_select(c, n, l1, req, &nn);
    if (voxel && voxel_scheduled(c)) { // (the level word: enqueue_fresh_states knows nothing of it)
        const int lvl = c->vox_step_level >= 0 && c->vox_step_level < c->vox_levels ? c->vox_step_level : c->vox_levels - 1;
        hipLaunchKernelGGL(voxel_sched_reset_kernel, dim3(1), dim3(64), 0, c->stream, c->d_state.get(), c->d_vox_sched.get(), (unsigned)lvl);
    }
    if (voxel) enqueue_voxel_solve(c, n, l1, d_Tstep, d_sums, true, false);
    else if (s == ICPMI_OK) {
        enqueue_accumulate_solve(c, n, l1, req.batch, nn, d_Tstep, d_sums);
        if (l1.degen) (void)loop_degen_report(c, l1); // (an error state leaves the sums of an earlier call: degen_ready stays false below)
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState), hipMemcpyDeviceToHost, c->stream);
    float hT[16]; double hS[ICPMI_NV];
    if (e == hipSuccess) e = hipMemcpyAsync(hT, d_Tstep, sizeof hT, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hS, d_sums, sizeof hS, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (s != ICPMI_OK) return s;
    HIP_TRY(c, e);
    fill_stats(c->h_state, l1, n, stats);
    if (c->h_state->error) { c->last_error = "minimize_step: device-side convergence error"; return (icpmi_status)c->h_state->error; }
    if (T_step) memcpy(T_step, hT, sizeof hT);
    if (sums) memcpy(sums, hS, sizeof hS);
    c->degen_ready = l1.degen != 0;
    return ICPMI_OK;
}

icpmi_status loop_upload_read_normals(icpmi_ctx* c, const float* normals3, int64_t n)
{
    float* d_n3 = scratch_get<float>(c, 9, (size_t)3 * n + 3);
    if (!d_n3 || c->d_read_normals.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(d_n3, normals3, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pad_normals_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, (const float*)d_n3, n, c->d_read_normals);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (pageable host memory: the caller's buffer is free on return)
    return ICPMI_OK;
}

// ---------------------------------------------------------------------------------------------
// ErrorMinimizer::getResidualError() under a given pose (include/icpmi.h: icpmi_residual_error has the formulation).  The state is set up
// as loop_single_step sets it up, the matcher's launch and the selection are the ones of a registration's first iteration; in place of the
// pair sums and the solve, two launches outside any graph: pass 1 walks the n * k slots and every workgroup writes five partials (sum r,
// sum r^2, sum w, pairs in double; max r), pass 2 (one workgroup) adds them in a fixed order.  No atomics: the same bits on every call.
// ---------------------------------------------------------------------------------------------
#define ICPMI_RES_NB 256   // pass-1 workgroups, one per CU (fixed, as ICPMI_COV_NB: the summation order depends on the slot count alone)
#define ICPMI_RES_NV 5     // [0] sum r, [1] sum r^2, [2] sum w, [3] pairs, [4] max r
#define ICPMI_RES_CH 8     // pass 2: eight threads per value, each over every eighth workgroup partial
#define ICPMI_RES_MAX (1u << 4) // the slots that combine with fmax

struct ResBlock { double sum_abs, sum_sq, weight_sum; long long pairs; float max_abs, limit; int error, pad; };

// fused_slot >= 0: the chain's one quantile filter went through the fused selection, whose last level the pair-sum kernel of an iteration
// resolves -- here every workgroup does (the same lookup, the same limit)
// blockIdx.y = pose of a batch (icpmi_residual_error_poses: one slice of the per-query arrays, one IcpState, one set of histograms and one
// row of ICPMI_RES_NB partials per pose); a single call is the batch of one, so a pose is scored to the same bits alone or among others
__global__ __launch_bounds__(256) void res_pairs_kernel(PairView pv, BatchArgs ba, LoopCfg lc, int kind, int planar, IcpState* __restrict__ st,
                                                        const unsigned* __restrict__ hists, int fused_slot, int is_median, float factor,
                                                        double* __restrict__ partial)
{
    const int n = ba.n[blockIdx.y];
    pair_view_slice(pv, ba, lc.k);
    hists += (size_t)blockIdx.y * ICPMI_SELHIST_WORDS;
    partial += (size_t)blockIdx.y * (ICPMI_RES_NB * ICPMI_RES_NV);
    st += blockIdx.y;
    __shared__ unsigned shsel[16];
    float fused_limit = 0.f;
    if (fused_slot >= 0) {
        const unsigned cv = hists[ICPMI_S2_C1 + threadIdx.x];
        unsigned bin, rem, total;
        block_find_rank_2tier<1>(cv, hists + ICPMI_S2_F1, false, 0.f, st->sel_rank_l[0], shsel, bin, rem, total);
        const float q = __uint_as_float((st->sel_prefix_l[0] << 16) | bin);
        fused_limit = is_median ? factor * q : q;
        if (blockIdx.x == 0 && threadIdx.x == 0) st->limits[fused_slot] = fused_limit;
    }
    double sr = 0.0, sq = 0.0, sw = 0.0, cnt = 0.0;
    float mx = 0.f;
    const bool have_n = pv.ref_normals != nullptr;
    if (st->error == 0) // (otherwise a selection that found nothing to filter: the partials are written, all zero)
        walk_pairs(pv, n, lc, st, st->T_iter, [&](const PairSlot& a) {
            if (a.w == 0.f) return;
            const float dot2 = have_n ? a.dx * a.nm.x + a.dy * a.nm.y : 0.f; // forcedDim = 2
            const float r = kind == ICPMI_RES_POINT_TO_POINT ? sqrtf(a.d2) : fabsf(planar ? dot2 : a.dot);
            sr += (double)r; sq += (double)r * (double)r; sw += (double)a.w; cnt += 1.0;
            mx = fmaxf(mx, r);
        }, fused_slot, fused_limit);
    const double acc[ICPMI_RES_NV] = {sr, sq, sw, cnt, (double)mx};
    block_partial_row<ICPMI_RES_NV, ICPMI_RES_MAX>(acc, partial + (size_t)blockIdx.x * ICPMI_RES_NV);
}

// blockIdx.x = pose of a batch: its row of partials, its IcpState, its ResBlock
__global__ __launch_bounds__(64) void res_finish_kernel(const double* __restrict__ partial, const IcpState* __restrict__ st, int limit_slot,
                                                        ResBlock* __restrict__ out)
{
    partial += (size_t)blockIdx.x * (ICPMI_RES_NB * ICPMI_RES_NV);
    st += blockIdx.x;
    out += blockIdx.x;
    __shared__ double tot[ICPMI_RES_NV];
    block_ordered_total<ICPMI_RES_NV, ICPMI_RES_CH, ICPMI_RES_NB, ICPMI_RES_MAX>(partial, ICPMI_RES_NB, tot);
    if (threadIdx.x != 0) return;
    out->sum_abs = tot[0]; out->sum_sq = tot[1]; out->weight_sum = tot[2];
    out->pairs = (long long)tot[3];
    out->max_abs = (float)tot[4];
    out->limit = limit_slot >= 0 ? st->limits[limit_slot] : -1.f;
    out->error = st->error; out->pad = 0;
}
static_assert(ICPMI_RES_NB % ICPMI_RES_CH == 0 && ICPMI_RES_NV * ICPMI_RES_CH <= 64, "pass 2 of the residual: one wave, whole chunks");

// what a call answers from a pose's result block: the convergence errors of a registration's first iteration, or the residual
static icpmi_status res_block_out(icpmi_ctx* c, const ResBlock& hr, int k, int64_t n, int kind, icpmi_residual* out)
{
    if (hr.error) {
        c->last_error = hr.error == ICPMI_ERR_NO_OUTLIER_TO_FILTER ? "ConvergenceError: no outlier to filter" : "residual_error: device-side convergence error";
        return (icpmi_status)hr.error;
    }
    if (hr.pairs <= 0) { c->last_error = "ConvergenceError: ErrorMinimizer: no point to minimize"; return ICPMI_ERR_NO_POINT_TO_MINIMIZE; }
    out->sum_abs = hr.sum_abs; out->sum_sq = hr.sum_sq; out->max_abs = hr.max_abs;
    out->weight_sum = hr.weight_sum; out->pairs = hr.pairs;
    out->weighted_point_used_ratio = (float)(hr.weight_sum / ((double)k * (double)n));
    out->trimmed_limit = hr.limit;
    out->kind = kind;
    return ICPMI_OK;
}

// the two passes behind enqueue_match_select: the partials of ba's poses into d_part, their result blocks into d_res (one per pose)
static icpmi_status enqueue_residual_sums(icpmi_ctx* c, const BatchArgs& ba, const LoopCfg& l1, int kind, int planar, const NnOutcome& nn, double* d_part,
                                          ResBlock* d_res)
{
    const int slot = fused_filter_slot(l1);
    hipLaunchKernelGGL(res_pairs_kernel, dim3(ICPMI_RES_NB, ba.nscan), dim3(256), 0, c->stream, pair_view(c, l1, nn.out_sorted), ba, l1, kind, planar,
                       c->d_state, (const unsigned*)c->d_selhist, slot >= 0 ? slot : -1,
                       (slot >= 0 && l1.out_type[slot] == ICPMI_OUT_MEDIANDIST) ? 1 : 0, slot >= 0 ? l1.out_param[slot] : 0.f, d_part);
    hipLaunchKernelGGL(res_finish_kernel, dim3(ba.nscan), dim3(64), 0, c->stream, (const double*)d_part, (const IcpState*)c->d_state, quantile_slot(l1), d_res);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// the centred reading is in c->d_reading (loop_prepare_reading); T_host = the pose in the centred frame (column-major), kind 1 or 2
icpmi_status loop_residual(icpmi_ctx* c, int64_t n, const LoopCfg& lc, const float T_host[16], int kind, int planar, const float* d_r2row,
                           icpmi_residual* out)
{
    // the covariance of the registration before this call lives in d_cov, which nothing here touches: it stays readable
    const bool cov_keep = c->cov_ready && (c->last_match_n != 0 || c->cov_kept);
    if (ensure_loop_buffers(c, n, lc) != ICPMI_OK) return ICPMI_ERR_HIP;
    // scratch 5: the partials, the result block, the pose
    constexpr size_t RES_DOUBLES = (sizeof(ResBlock) + sizeof(double) - 1) / sizeof(double);
    double* d_part = scratch_get<double>(c, 5, (size_t)ICPMI_RES_NB * ICPMI_RES_NV + RES_DOUBLES + 8);
    if (!d_part) return ICPMI_ERR_HIP;
    ResBlock* d_res = reinterpret_cast<ResBlock*>(d_part + ICPMI_RES_NB * ICPMI_RES_NV);
    float* d_T0 = reinterpret_cast<float*>(d_part + ICPMI_RES_NB * ICPMI_RES_NV + RES_DOUBLES);
    { const icpmi_status us = upload_small(c, d_T0, T_host, 16 * sizeof(float)); if (us != ICPMI_OK) return us; }
    { const icpmi_status is = enqueue_fresh_states(c, 1, d_T0); if (is != ICPMI_OK) return is; }
    const LoopCfg l1 = one_pass_cfg(lc);
    const NnRequest req = loop_request(c, l1, batch_of_one(n), d_r2row); // (iter 0: what a registration's first iteration asks of the matcher)
    NnOutcome nn;
    { const icpmi_status s = enqueue_match_select(c, n, l1, req, &nn); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = enqueue_residual_sums(c, req.batch, l1, kind, planar, nn, d_part, d_res); if (s != ICPMI_OK) return s; }
    ResBlock hr;
    if (read_back(c, &hr, d_res, sizeof hr) != ICPMI_OK) return ICPMI_ERR_HIP;
    c->cov_kept = cov_keep; // (the matcher's launch dropped last_match_n: icpmi_debug_last_matches has nothing to read any more)
    return res_block_out(c, hr, l1.k, n, kind, out);
}

// slices 1 .. gridDim.y of the tile-sorted reading and its index row from slice 0 (the pose batch: one reading, centred and sorted once)
__global__ __launch_bounds__(256) void res_replicate_kernel(float4* __restrict__ qsorted, int* __restrict__ qindex, int n, int qstride)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t o = (size_t)(blockIdx.y + 1) * (size_t)qstride + i;
    qsorted[o] = qsorted[i];
    qindex[o] = qindex[i];
}

// icpmi_residual_error_poses on the batched route (api.hip decides which chains take it: the ones icpmi_register_batch_dev runs together).
// The centred reading of n points is in c->d_reading (nothing prepared yet: this function centres and sorts it once, after its
// allocations); T_host = n_poses poses in the centred frame.  Chunks of up to ICPMI_MAX_BATCH poses go through the launches of
// loop_residual with blockIdx.y = pose, back to back; one read-back of the n_poses result blocks ends the call.
icpmi_status loop_residual_poses(icpmi_ctx* c, const float4* d_scan, int64_t n, const LoopCfg& lc, const float* T_host, int n_poses, int kind,
                                 int planar, icpmi_residual* out, icpmi_status* status)
{
    const bool cov_keep = c->cov_ready && (c->last_match_n != 0 || c->cov_kept);
    const int B = n_poses < ICPMI_MAX_BATCH ? n_poses : ICPMI_MAX_BATCH;
    const int64_t NS = (n + 63) / 64 * 64; // slice stride of the per-query arrays, as loop_run_batch
    // all allocations before the first launch (a later one could move the sorted reading)
    if (ensure_loop_buffers(c, NS, lc, B) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (c->d_reading.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (sort_queries_reserve(c, NS, B) != ICPMI_OK) return ICPMI_ERR_HIP;
    // scratch 5: the partials of one chunk, then per pose its result block and its pose
    constexpr size_t RES_DOUBLES = (sizeof(ResBlock) + sizeof(double) - 1) / sizeof(double);
    static_assert(sizeof(ResBlock) % sizeof(double) == 0, "an array of result blocks behind the partials");
    const size_t part_doubles = (size_t)B * ICPMI_RES_NB * ICPMI_RES_NV;
    double* d_part = scratch_get<double>(c, 5, part_doubles + (size_t)n_poses * (RES_DOUBLES + 8) + 8);
    if (!d_part) return ICPMI_ERR_HIP;
    ResBlock* d_res = reinterpret_cast<ResBlock*>(d_part + part_doubles);
    float* d_T = reinterpret_cast<float*>(d_part + part_doubles + (size_t)n_poses * RES_DOUBLES);
    std::vector<ResBlock> hr((size_t)n_poses);

    { const icpmi_status ps = loop_prepare_reading(c, d_scan, n, nullptr); if (ps != ICPMI_OK) return ps; }
    HIP_TRY(c, hipMemcpyAsync(d_T, T_host, (size_t)n_poses * 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (B > 1)
        hipLaunchKernelGGL(res_replicate_kernel, dim3((int)((n + 255) / 256), B - 1), dim3(256), 0, c->stream, c->d_qsorted.get(), c->d_qindex.get(),
                           (int)n, (int)NS);
    const LoopCfg l1 = one_pass_cfg(lc);
    for (int p0 = 0; p0 < n_poses; p0 += B) {
        const int Bc = n_poses - p0 < B ? n_poses - p0 : B;
        BatchArgs ba; memset(&ba, 0, sizeof ba);
        ba.nscan = Bc; ba.qstride = Bc > 1 ? (int)NS : 0;
        for (int b = 0; b < Bc; ++b) ba.n[b] = (int)n;
        { const icpmi_status is = enqueue_fresh_states(c, Bc, d_T + 16 * (size_t)p0); if (is != ICPMI_OK) return is; }
        const NnRequest req = loop_request(c, l1, ba, nullptr); // (iter 0: what a registration's first iteration asks of the matcher)
        NnOutcome nn;
        { const icpmi_status s = enqueue_match_select(c, n, l1, req, &nn); if (s != ICPMI_OK) return s; }
        { const icpmi_status s = enqueue_residual_sums(c, ba, l1, kind, planar, nn, d_part, d_res + p0); if (s != ICPMI_OK) return s; }
    }
    if (read_back(c, hr.data(), d_res, sizeof(ResBlock) * (size_t)n_poses) != ICPMI_OK) return ICPMI_ERR_HIP;
    c->cov_kept = cov_keep;
    for (int p = 0; p < n_poses; ++p) status[p] = res_block_out(c, hr[(size_t)p], l1.k, n, kind, out + p);
    return ICPMI_OK;
}

icpmi_status loop_outlier_weights(icpmi_ctx* c, const LoopCfg& lc, const float* d2, const int32_t* ids, int k, int64_t n,
                                  const float* read_normals3, float* weights, float* limit_out)
{
    c->last_match_n = 0; c->cov_kept = false; // (d2 / ids of the caller go through the loop's buffers)
    // matches arrive with ORIGINAL ids; the device's normals table is in sorted order.  SurfaceNormalOutlierFilter (r4) reads the map's
    // normals from the resident copy instead, which IS in the caller's order (d_raw_n3, padded to float4 for the kernel).
    bool needs_sn = false;
    for (int f = 0; f < lc.n_out; ++f) needs_sn |= lc.out_type[f] == ICPMI_OUT_SURFACENORMAL;
    float4* d_ref_n4 = nullptr;
    float* d_rn3 = nullptr;
    if (needs_sn) {
        if (!ids || !read_normals3 || !c->raw_has_normals || c->m_raw <= 0) {
            c->last_error = "InvalidField: SurfaceNormalOutlierFilter needs ids, 'normals' on the reading and 'normals' on the map";
            return ICPMI_ERR_MISSING_NORMALS;
        }
        for (int64_t e = 0; e < (int64_t)k * n; ++e)
            if (ids[e] >= c->m_raw) { c->last_error = "outlier_weights: id outside the map"; return ICPMI_ERR_INVALID_ARG; }
        d_ref_n4 = scratch_get<float4>(c, 8, (size_t)c->m_raw + 1);
        d_rn3 = scratch_get<float>(c, 9, (size_t)3 * n + 3);
        if (!d_ref_n4 || !d_rn3) return ICPMI_ERR_HIP;
        if (c->d_read_normals.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(c, hipMemcpyAsync(d_rn3, read_normals3, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(pad_normals_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, (const float*)d_rn3, n, c->d_read_normals);
        hipLaunchKernelGGL(pad_normals_kernel, dim3((int)((c->m_raw + 255) / 256)), dim3(256), 0, c->stream, (const float*)c->d_raw_n3, c->m_raw, d_ref_n4);
        HIP_TRY(c, hipGetLastError());
    }
    bool needs_ids = false;
    for (int f = 0; f < lc.n_out; ++f) {
        if (lc.out_type[f] == ICPMI_OUT_ROBUST && ((lc.out_iparam[f] >> 8) & 15) == ICPMI_DIST_POINT2PLANE) {
            c->last_error = "icpmi_outlier_weights: RobustOutlierFilter{distanceType: point2plane} is only available inside icpmi_register";
            return ICPMI_ERR_UNSUPPORTED;
        }
        if (lc.out_type[f] == ICPMI_OUT_GENERICDESCRIPTOR) {
            if (!ids || !c->raw_has_scalar) { c->last_error = "InvalidField: GenericDescriptorOutlierFilter needs ids and the tracked scalar descriptor on the map"; return ICPMI_ERR_INVALID_ARG; }
            for (int64_t e = 0; e < (int64_t)k * n; ++e)
                if (ids[e] >= c->m_raw) { c->last_error = "outlier_weights: id outside the map"; return ICPMI_ERR_INVALID_ARG; }
        }
        needs_ids |= lc.out_type[f] == ICPMI_OUT_GENERICDESCRIPTOR || lc.out_type[f] == ICPMI_OUT_ROBUST || lc.out_type[f] == ICPMI_OUT_SURFACENORMAL;
    }
    const int64_t count = (int64_t)k * n;
    LoopCfg l1 = lc; l1.k = k;
    if (ensure_loop_buffers(c, n, l1) != ICPMI_OK) return ICPMI_ERR_HIP;
    { const icpmi_status is = enqueue_fresh_states(c, 1, nullptr); if (is != ICPMI_OK) return is; }
    HIP_TRY(c, hipMemcpyAsync(c->d_d2, d2, (size_t)count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (needs_ids && ids) HIP_TRY(c, hipMemcpyAsync(c->d_sidx, ids, (size_t)count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    else HIP_TRY(c, hipMemsetAsync(c->d_sidx, 0, (size_t)count * sizeof(int), c->stream));
    enqueue_selection(c, l1, count, batch_of_one(n), NnOutcome(), true); // (no matcher launch in front: the caller's d2)
    DevBuf<float> d_w;
    HIP_TRY(c, d_w.alloc((size_t)count));
    const int blocks = (int)((count + 255) / 256);
    if (blocks) hipLaunchKernelGGL(weights_kernel, dim3(blocks), dim3(256), 0, c->stream, count, l1, c->d_state,
                                   needs_sn ? (const float4*)d_ref_n4 : (const float4*)c->d_normals_sorted,
                                   needs_sn ? (const float4*)c->d_read_normals : (const float4*)nullptr, c->d_sidx, c->d_d2, d_w,
                                   c->raw_has_scalar ? c->d_raw_s : (const float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(weights, d_w, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->h_state, c->d_state, sizeof(IcpState), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIP_TRY(c, e);
    if (c->h_state->error) { c->last_error = "ConvergenceError: no outlier to filter"; return (icpmi_status)c->h_state->error; }
    if (limit_out) {
        *limit_out = -1.f;
        const int q = quantile_slot(l1); // (... or the scale of a Robust filter behind it)
        for (int f = 0; f < l1.n_out; ++f)
            if (f == q) *limit_out = c->h_state->limits[f];
            else if (l1.out_type[f] == ICPMI_OUT_ROBUST && ((l1.out_iparam[f] >> 4) & 15) != ICPMI_SCALE_NONE) *limit_out = c->h_state->robust_scale;
    }
    return ICPMI_OK;
}
