// normalspace.hip -- NormalSpaceDataPointsFilter{nbSample, seed, epsilon} on the device (libpointmatcher DataPointsFilters/NormalSpace.cpp,
// Rusinkiewicz & Levoy 2001, as recalled: its source is not vendored; the formulation is written down in include/icpmi.h next to
// icpmi_normal_space_sampling and in INTEGRATION.md).
//
// Every point falls into an angular bucket of its normal (theta = acos(nz), phi = atan2(ny, nx) in [0, 2 pi], epsilon wide) and gets a
// random number r_i, the (i + 1)-th value of std::minstd_rand(seed).  The buckets are visited round-robin in ascending index, one
// point per non-empty bucket per round in ascending r_i, until nbSample points are taken.  In closed form: with c_b the population of
// bucket b and S(R) = sum_b min(c_b, R), R* = the largest R with S(R) <= nbSample; every point of rank < R* in its bucket is kept, and
// the points of rank R* in the first nbSample - S(R*) buckets that have one.  Here:
//   1. ns_key_kernel: bucket and r_i per point, the sort pair (bucket << 31 | r_i, i), the non-finite flag;
//   2. one stable LSD radix sort of the pairs (31 + log2(buckets) key bits): every bucket contiguous, in ascending r_i;
//   3. ns_bounds_kernel: first and one-past-last sorted position of every non-empty bucket (c_b = their difference);
//   4. ns_search_kernel: ONE workgroup holds the <= 2^14 counts in LDS, bisects R*, and writes how many points every bucket gives
//      (R*, or R* + 1 for the first `rem` buckets with c_b > R*: a prefix count over the buckets);
//   5. ns_flag_kernel: sorted position -> rank in its bucket -> keep flag at the point's ORIGINAL index;
//   6. the flag scan and ns_emit_kernel: the kept indices in ascending order.
// No atomics at all (the counts come from the sorted order; the non-finite flag is a plain store of 1 by whoever sees one): two calls
// give the same bits.  The only host wait is the final one (order, buckets and the status word).
#include "common.h"

namespace {

constexpr int NB = 256;
constexpr unsigned NS_MAX_BUCKETS = 1u << 14; // epsilon >= 0.04908: at most 65 rows of 128 columns + 1

struct NsDev {
    int nonfinite;       // a coordinate or a normal component is not finite
    unsigned rstar, rem; // R* and nbSample - S(R*)
    unsigned pad;
};

__device__ __forceinline__ bool ns_finite(float v) { return finite_within(v, 3.402823466e38f); }

// per point: bucket = floorf(theta / eps) * stride + floorf(phi / eps) (float32; the angles go through double and are rounded once),
// the sort pair and -- bucket_out != null -- the bucket itself
__global__ __launch_bounds__(NB) void ns_key_kernel(const float4* __restrict__ pts, const float* __restrict__ nrm, int64_t n, float eps, unsigned stride,
                                                    unsigned nbuckets, unsigned seed, unsigned long long* __restrict__ keys,
                                                    unsigned* __restrict__ vals, int* __restrict__ bucket_out, NsDev* __restrict__ d)
{
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
    if (!(ns_finite(p.x) && ns_finite(p.y) && ns_finite(p.z) && ns_finite(nx) && ns_finite(ny) && ns_finite(nz))) d->nonfinite = 1;
    const float cz = fminf(fmaxf(nz, -1.f), 1.f);
    const float theta = (float)acos((double)cz);
    double pd = atan2((double)ny, (double)nx);
    if (pd < 0.0) pd = pd + 6.283185307179586;
    const float phi = (float)pd;
    const unsigned bt = (unsigned)floorf(theta / eps), bp = (unsigned)floorf(phi / eps);
    unsigned b = bt * stride + bp;
    b = b < nbuckets ? b : nbuckets - 1u; // (finite normals never get here: the table is sized from the largest theta and phi; NaN may)
    keys[i] = ((unsigned long long)b << 31) | (unsigned long long)minstd_nth(seed, (unsigned)i + 1u);
    vals[i] = (unsigned)i;
    if (bucket_out) bucket_out[i] = (int)b;
}

// over the sorted pairs: first[b] = the first position of bucket b, last[b] = one past its last (both 0 for an empty bucket)
__global__ __launch_bounds__(NB) void ns_bounds_kernel(const unsigned long long* __restrict__ keys, int64_t n, unsigned* __restrict__ first,
                                                       unsigned* __restrict__ last)
{
    const int64_t j = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (j >= n) return;
    const unsigned b = (unsigned)(keys[j] >> 31);
    if (j == 0 || (unsigned)(keys[j - 1] >> 31) != b) first[b] = (unsigned)j;
    if (j == n - 1 || (unsigned)(keys[j + 1] >> 31) != b) last[b] = (unsigned)j + 1u;
}

// sum / max of one unsigned per thread over the workgroup (NB = 4 waves), the result in every thread; `slot` alternates between
// consecutive calls so that one barrier per call is enough
template <bool MAX>
__device__ __forceinline__ unsigned ns_block_reduce(unsigned v, unsigned (*red)[NB / 64], int slot)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned o = __shfl_xor(v, off, 64);
        v = MAX ? (o > v ? o : v) : v + o;
    }
    if ((threadIdx.x & 63) == 0) red[slot][threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned r = red[slot][0];
#pragma unroll
    for (int w = 1; w < NB / 64; ++w) r = MAX ? (red[slot][w] > r ? red[slot][w] : r) : r + red[slot][w];
    return r;
}

// ONE workgroup: c_b = last[b] - first[b] in LDS; R* by bisection (S(0) = 0 <= nb < n = S(max c): at most 31 steps); take[b] = how
// many points bucket b gives, in ascending r_i: R*, and one more for the first `rem` buckets, in ascending index, among those with
// c_b > R* (there are more than `rem` of them, or R* + 1 would have fitted)
__global__ __launch_bounds__(NB) void ns_search_kernel(const unsigned* __restrict__ first, const unsigned* __restrict__ last, unsigned nbuckets, unsigned nb,
                                                       unsigned* __restrict__ take, NsDev* __restrict__ d)
{
    __shared__ unsigned sc[NS_MAX_BUCKETS];
    __shared__ unsigned red[2][NB / 64];
    __shared__ unsigned above[NB];
    const unsigned t = threadIdx.x;
    unsigned mx = 0u;
    for (unsigned b = t; b < nbuckets; b += NB) {
        const unsigned c = last[b] - first[b];
        sc[b] = c;
        mx = c > mx ? c : mx;
    }
    int slot = 0;
    unsigned hi = ns_block_reduce<true>(mx, red, slot); // (its barrier also publishes sc)
    slot ^= 1;
    unsigned lo = 0u, slo = 0u;
    while (hi - lo > 1u) {
        const unsigned mid = lo + (hi - lo) / 2u;
        unsigned s = 0u;
        for (unsigned b = t; b < nbuckets; b += NB) s += sc[b] < mid ? sc[b] : mid;
        s = ns_block_reduce<false>(s, red, slot);
        slot ^= 1;
        if (s <= nb) { lo = mid; slo = s; }
        else hi = mid;
    }
    const unsigned rem = nb - slo;
    // thread t owns the buckets [t per, (t + 1) per): how many of them have a point of rank R*, then how many such buckets come before
    const unsigned per = (nbuckets + NB - 1u) / NB;
    const unsigned b0 = t * per < nbuckets ? t * per : nbuckets;
    const unsigned b1 = b0 + per < nbuckets ? b0 + per : nbuckets;
    unsigned mine = 0u;
    for (unsigned b = b0; b < b1; ++b) mine += sc[b] > lo ? 1u : 0u;
    above[t] = mine;
    __syncthreads();
    unsigned before = 0u;
    for (unsigned u = 0; u < t; ++u) before += above[u];
    for (unsigned b = b0; b < b1; ++b) {
        const bool has = sc[b] > lo;
        take[b] = lo + ((has && before < rem) ? 1u : 0u);
        before += has ? 1u : 0u;
    }
    if (t == 0) { d->rstar = lo; d->rem = rem; }
}

// sorted position j -> the point's rank in its bucket -> keep flag at its original index
__global__ __launch_bounds__(NB) void ns_flag_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals, int64_t n,
                                                     const unsigned* __restrict__ first, const unsigned* __restrict__ take, unsigned* __restrict__ flag)
{
    const int64_t j = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (j >= n) return;
    const unsigned b = (unsigned)(keys[j] >> 31);
    flag[vals[j]] = ((unsigned)j - first[b]) < take[b] ? 1u : 0u;
}

// pos = exclusive scan of the flags: the kept indices in ascending order
__global__ __launch_bounds__(NB) void ns_emit_kernel(int64_t n, const unsigned* __restrict__ flag, const unsigned* __restrict__ pos, int64_t cap,
                                                     int* __restrict__ order)
{
    const int64_t i = (int64_t)blockIdx.x * NB + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const unsigned o = pos[i];
    if ((int64_t)o < cap) order[o] = (int)i;
}

} // namespace

// the number of buckets the two floors can reach: theta <= (float)pi, phi <= (float)(2 pi), float division is monotonic
static unsigned ns_table(float eps, unsigned* stride)
{
    const float fs = floorf(6.2831855f / eps), ft = floorf(3.14159274f / eps);
    *stride = (unsigned)fs;
    return (unsigned)ft * (unsigned)fs + (unsigned)fs + 1u;
}

// 0 < nb < n, normals3 != null (icpmi_normal_space_sampling has dealt with the rest)
icpmi_status ops_normal_space_sampling(icpmi_ctx* c, const float* in4, int64_t n, const float* normals3, int64_t nb, unsigned seed, float eps,
                                       int32_t* order_out, int32_t* bucket_out)
{
    unsigned stride = 0;
    const unsigned nbuckets = ns_table(eps, &stride);
    if (stride == 0u || nbuckets > NS_MAX_BUCKETS) { c->last_error = "normal_space_sampling: epsilon gives too many buckets"; return ICPMI_ERR_INVALID_ARG; }
    int bbits = 1;
    while ((1u << bbits) < nbuckets) ++bbits;
    const int bits = 31 + bbits;
    const int blocks = (int)((n + NB - 1) / NB);
    DevBuf<float4> d_in; DevBuf<float> d_nrm; DevBuf<int> d_order, d_bucket;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_nrm.alloc((size_t)3 * n));
    HIP_TRY(c, d_order.alloc((size_t)nb));
    if (bucket_out) HIP_TRY(c, d_bucket.alloc((size_t)n));
    unsigned long long* d_keys = scratch_get<unsigned long long>(c, 0, (size_t)2 * n + 2);
    unsigned* d_vals = scratch_get<unsigned>(c, 1, (size_t)2 * n + 2);
    unsigned* d_tab = scratch_get<unsigned>(c, 2, radix_sort_tab_words(n, bits));
    const size_t dev_words = (sizeof(NsDev) + sizeof(unsigned) - 1) / sizeof(unsigned);
    unsigned* d_small = scratch_get<unsigned>(c, 3, (size_t)3 * nbuckets + dev_words);
    unsigned* d_flag = scratch_get<unsigned>(c, 4, (size_t)2 * n + 4);
    if (!d_keys || !d_vals || !d_tab || !d_small || !d_flag) return ICPMI_ERR_HIP;
    unsigned* d_first = d_small;
    unsigned* d_last = d_small + nbuckets;
    unsigned* d_take = d_small + 2 * (size_t)nbuckets;
    NsDev* d_dev = reinterpret_cast<NsDev*>(d_small + 3 * (size_t)nbuckets);
    unsigned* d_pos = d_flag + n + 2; // n + 1 words: the scan writes its total behind the positions

    HIP_TRY(c, hipMemcpyAsync(d_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_nrm, normals3, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_small, 0, ((size_t)3 * nbuckets + dev_words) * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(ns_key_kernel, dim3(blocks), dim3(NB), 0, c->stream, (const float4*)d_in, (const float*)d_nrm, n, eps, stride, nbuckets, seed, d_keys,
                       d_vals, bucket_out ? d_bucket.get() : (int*)nullptr, d_dev);
    HIP_TRY(c, hipGetLastError());
    int half = 0;
    const icpmi_status ss = radix_sort_pairs(c, d_keys, d_vals, n, bits, d_tab, &half);
    if (ss != ICPMI_OK) return ss;
    // radix_sort_pairs' halves are [0, n) and [n, 2 n) of the arrays
    const unsigned long long* skeys = d_keys + (half ? n : 0);
    const unsigned* svals = d_vals + (half ? n : 0);
    hipLaunchKernelGGL(ns_bounds_kernel, dim3(blocks), dim3(NB), 0, c->stream, skeys, n, d_first, d_last);
    hipLaunchKernelGGL(ns_search_kernel, dim3(1), dim3(NB), 0, c->stream, (const unsigned*)d_first, (const unsigned*)d_last, nbuckets, (unsigned)nb, d_take,
                       d_dev);
    hipLaunchKernelGGL(ns_flag_kernel, dim3(blocks), dim3(NB), 0, c->stream, skeys, svals, n, (const unsigned*)d_first, (const unsigned*)d_take, d_flag);
    HIP_TRY(c, hipGetLastError());
    const icpmi_status sc = device_exclusive_scan_io(c, d_flag, d_pos, (int)n, 0u);
    if (sc != ICPMI_OK) return sc;
    hipLaunchKernelGGL(ns_emit_kernel, dim3(blocks), dim3(NB), 0, c->stream, n, (const unsigned*)d_flag, (const unsigned*)d_pos, nb, (int*)d_order);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(order_out, d_order, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (bucket_out) HIP_TRY(c, hipMemcpyAsync(bucket_out, d_bucket, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    NsDev h;
    if (read_back(c, &h, d_dev, sizeof h) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (h.nonfinite) { c->last_error = "normal_space_sampling: the cloud has non-finite coordinates or normals"; return ICPMI_ERR_INVALID_ARG; }
    return ICPMI_OK;
}
