// covsampling.hip -- CovarianceSamplingDataPointsFilter{nbSample, torqueNorm} on the device (libpointmatcher
// DataPointsFilters/CovarianceSampling.cpp, Gelfand et al. 2003, as recalled: its source is not vendored; the formulation is written
// down in include/icpmi.h next to icpmi_covariance_sampling and in INTEGRATION.md).
//
// Every point gets v = [ (1/L) ((p - c) x n) ; n ]; C = sum v v^T; x_0 .. x_5 = the eigenvectors of C in ascending eigenvalue order.
// List k holds every point sorted by |v . x_k| descending (stable); a greedy loop picks, nbSample times, the first unselected point of
// the list whose accumulated t_k = sum over the picks of (v . x_k)^2 is smallest.  Here:
//   1. cs_moments_kernel -> cs_center_kernel: the centre (double sums), the bounding box and a non-finite count;
//   2. cs_dist_kernel -> cs_lnorm_kernel: L (mean distance to the centre for torqueNorm 1);
//   3. cs_cov_kernel -> cs_eigen_kernel: the 21 unique entries of C, then a one-lane cyclic Jacobi in double and a stable ascending sort
//      of the eigenpairs;
//   4. cs_key_kernel: the six keys ~bits((float)|v . x_k|) (descending order = ascending key, the keys are >= 0) and the six weights
//      (v . x_k)^2 per point;
//   5. one stable LSD radix sort of (list << 32 | key, index) over all six lists at once (35 key bits; ties keep ascending index);
//   6. cs_greedy_kernel: one wave runs the nbSample steps (below).
// Every sum is per-thread sequential, then a fixed tree over the workgroup, then a fixed-order sum over the workgroups: no float
// atomics, two calls give the same bits.  The only host wait is the final one (order, info and the status word).
#include "common.h"

namespace {

constexpr int CB = 256;
constexpr int CS_MAX_PARTS = 1024;
constexpr int CS_W = 64;                    // window: the next 64 entries of a list, one per lane
constexpr int64_t CS_LDS_POINTS = 1 << 20;  // the selected flags live in an LDS bitmap up to this many points (128 KiB)

struct CsDev {
    icpmi_covsamp_info info;
    double lmax;         // half the largest bounding-box extent
    int nonfinite;       // a coordinate or a normal component is not finite
    int exhausted;       // the greedy loop found a list without an unselected point (cannot happen for nbSample < N)
};

__device__ __forceinline__ bool cs_finite(float v) { return finite_within(v, 3.402823466e38f); }

// v = [ s ((p - c) x n) ; n ] in double, in the order of the formulation
__device__ __forceinline__ void cs_vec(const float4 p, const float* __restrict__ nrm, int64_t i, const double* c, double s, double (&v)[6])
{
    const double ax = (double)p.x - c[0], ay = (double)p.y - c[1], az = (double)p.z - c[2];
    const double bx = (double)nrm[3 * i], by = (double)nrm[3 * i + 1], bz = (double)nrm[3 * i + 2];
    const double tx = (ay * bz) - (az * by);
    const double ty = (az * bx) - (ax * bz);
    const double tz = (ax * by) - (ay * bx);
    v[0] = s * tx; v[1] = s * ty; v[2] = s * tz;
    v[3] = bx; v[4] = by; v[5] = bz;
}

// fixed-order tree over the workgroup of R doubles per thread (sh: R x CB); the sums end in sh[r][0]
template <int R>
__device__ __forceinline__ void cs_tree(double (*sh)[CB], const double (&a)[R])
{
    const int t = threadIdx.x;
#pragma unroll
    for (int r = 0; r < R; ++r) sh[r][t] = a[r];
    __syncthreads();
    for (int h = CB / 2; h > 0; h >>= 1) {
        if (t < h)
#pragma unroll
            for (int r = 0; r < R; ++r) sh[r][t] = sh[r][t] + sh[r][t + h];
        __syncthreads();
    }
}

// per workgroup: sums of x, y, z (double), min / max of x, y, z, and how many points have a non-finite coordinate or normal component
__global__ __launch_bounds__(CB) void cs_moments_kernel(const float4* __restrict__ pts, const float* __restrict__ nrm, int64_t n, double* __restrict__ part)
{
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        const float4 p = pts[i];
        const float nx = nrm[3 * i], ny = nrm[3 * i + 1], nz = nrm[3 * i + 2];
        a[0] = a[0] + (double)p.x; a[1] = a[1] + (double)p.y; a[2] = a[2] + (double)p.z;
        a[3] += (cs_finite(p.x) && cs_finite(p.y) && cs_finite(p.z) && cs_finite(nx) && cs_finite(ny) && cs_finite(nz)) ? 0.0 : 1.0;
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
    __shared__ double sh[4][CB];
    __shared__ float sl[3][CB], su[3][CB];
    const int t = threadIdx.x;
    for (int r = 0; r < 3; ++r) { sl[r][t] = lo[r]; su[r][t] = hi[r]; }
    cs_tree<4>(sh, a);
    for (int h = CB / 2; h > 0; h >>= 1) {
        if (t < h)
            for (int r = 0; r < 3; ++r) { sl[r][t] = fminf(sl[r][t], sl[r][t + h]); su[r][t] = fmaxf(su[r][t], su[r][t + h]); }
        __syncthreads();
    }
    if (t == 0) {
        double* o = part + 10 * blockIdx.x;
        for (int r = 0; r < 4; ++r) o[r] = sh[r][0];
        for (int r = 0; r < 3; ++r) { o[4 + r] = (double)sl[r][0]; o[7 + r] = (double)su[r][0]; }
    }
}

// one workgroup: c = sums / n, half the largest extent, the non-finite flag
__global__ __launch_bounds__(CB) void cs_center_kernel(const double* __restrict__ part, int nparts, int64_t n, CsDev* __restrict__ d)
{
    const int t = threadIdx.x;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int b = t; b < nparts; b += CB) {
        const double* o = part + 10 * b;
        for (int r = 0; r < 4; ++r) a[r] = a[r] + o[r];
        for (int r = 0; r < 3; ++r) { lo[r] = fmin(lo[r], o[4 + r]); hi[r] = fmax(hi[r], o[7 + r]); }
    }
    __shared__ double sh[4][CB];
    __shared__ double sl[3][CB], su[3][CB];
    for (int r = 0; r < 3; ++r) { sl[r][t] = lo[r]; su[r][t] = hi[r]; }
    cs_tree<4>(sh, a);
    for (int h = CB / 2; h > 0; h >>= 1) {
        if (t < h)
            for (int r = 0; r < 3; ++r) { sl[r][t] = fmin(sl[r][t], sl[r][t + h]); su[r][t] = fmax(su[r][t], su[r][t + h]); }
        __syncthreads();
    }
    if (t == 0) {
        const double dn = (double)n;
        double ext = 0.0;
        for (int r = 0; r < 3; ++r) {
            d->info.center[r] = sh[r][0] / dn;
            const double e = su[r][0] - sl[r][0];
            ext = e > ext ? e : ext;
        }
        d->lmax = 0.5 * ext;
        d->nonfinite = sh[3][0] != 0.0 ? 1 : 0;
        d->exhausted = 0;
    }
}

// per workgroup: sum of |p - c| (torqueNorm 1)
__global__ __launch_bounds__(CB) void cs_dist_kernel(const float4* __restrict__ pts, int64_t n, const CsDev* __restrict__ d, double* __restrict__ part)
{
    const double c0 = d->info.center[0], c1 = d->info.center[1], c2 = d->info.center[2];
    double a[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        const float4 p = pts[i];
        const double x = (double)p.x - c0, y = (double)p.y - c1, z = (double)p.z - c2;
        a[0] = a[0] + sqrt((x * x + y * y) + z * z);
    }
    __shared__ double sh[1][CB];
    cs_tree<1>(sh, a);
    if (threadIdx.x == 0) part[blockIdx.x] = sh[0][0];
}

// one workgroup: L of the torque norm; L == 0 (every point equal) -> 1
__global__ __launch_bounds__(CB) void cs_lnorm_kernel(const double* __restrict__ part, int nparts, int64_t n, int mode, CsDev* __restrict__ d)
{
    double a[1] = {0.0};
    if (mode == 1)
        for (int b = threadIdx.x; b < nparts; b += CB) a[0] = a[0] + part[b];
    __shared__ double sh[1][CB];
    cs_tree<1>(sh, a);
    if (threadIdx.x == 0) {
        double L = 1.0;
        if (mode == 1) L = sh[0][0] / (double)n;
        else if (mode == 2) L = d->lmax;
        d->info.lnorm = L == 0.0 ? 1.0 : L;
    }
}

// per workgroup: the 21 entries C[r][q], r <= q, of sum v v^T (row-major upper triangle)
__global__ __launch_bounds__(CB) void cs_cov_kernel(const float4* __restrict__ pts, const float* __restrict__ nrm, int64_t n, const CsDev* __restrict__ d,
                                                    double* __restrict__ part)
{
    const double c[3] = {d->info.center[0], d->info.center[1], d->info.center[2]};
    const double s = 1.0 / d->info.lnorm;
    double a[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) a[e] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x; i < n; i += (int64_t)gridDim.x * CB) {
        double v[6];
        cs_vec(pts[i], nrm, i, c, s, v);
        int e = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = r; q < 6; ++q) { a[e] = a[e] + v[r] * v[q]; ++e; }
    }
    __shared__ double sh[21][CB];
    cs_tree<21>(sh, a);
    if (threadIdx.x < 21) part[21 * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
}

// one workgroup: C from the partials, then lane 0: cyclic Jacobi (rotations as in Numerical Recipes' jacobi, rows and columns applied
// in full, the annihilated pair set to 0), eigenvalues sorted ascending by a stable insertion sort, basis[6 k + j] = x_k[j]
__global__ __launch_bounds__(CB) void cs_eigen_kernel(const double* __restrict__ part, int nparts, CsDev* __restrict__ d)
{
    double a[21];
#pragma unroll
    for (int e = 0; e < 21; ++e) a[e] = 0.0;
    for (int b = threadIdx.x; b < nparts; b += CB)
#pragma unroll
        for (int e = 0; e < 21; ++e) a[e] = a[e] + part[21 * b + e];
    __shared__ double sh[21][CB];
    cs_tree<21>(sh, a);
    if (threadIdx.x != 0) return;
    double A[6][6], V[6][6];
    {
        int e = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = r; q < 6; ++q) { A[r][q] = A[q][r] = sh[e][0]; ++e; }
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int q = 0; q < 6; ++q) V[r][q] = r == q ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) off += fabs(A[p][q]);
        if (!(off > 0.0)) break; // converged (or NaN input: the status word reports it)
#pragma unroll
        for (int p = 0; p < 6; ++p)
#pragma unroll
            for (int q = p + 1; q < 6; ++q) {
                const double apq = A[p][q];
                const double g = 100.0 * fabs(apq);
                if (sweep > 3 && fabs(A[p][p]) + g == fabs(A[p][p]) && fabs(A[q][q]) + g == fabs(A[q][q])) { A[p][q] = A[q][p] = 0.0; continue; }
                if (apq == 0.0) continue;
                const double h = A[q][q] - A[p][p];
                double tn;
                if (fabs(h) + g == fabs(h)) tn = apq / h;
                else {
                    const double theta = 0.5 * h / apq;
                    tn = 1.0 / (fabs(theta) + sqrt(1.0 + theta * theta));
                    if (theta < 0.0) tn = -tn;
                }
                const double cs = 1.0 / sqrt(tn * tn + 1.0), sn = tn * cs;
#pragma unroll
                for (int k = 0; k < 6; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = cs * x - sn * y; A[k][q] = sn * x + cs * y; }
#pragma unroll
                for (int k = 0; k < 6; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = cs * x - sn * y; A[q][k] = sn * x + cs * y; }
                A[p][q] = A[q][p] = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) { const double x = V[k][p], y = V[k][q]; V[k][p] = cs * x - sn * y; V[k][q] = sn * x + cs * y; }
            }
    }
    double ev[6];
    int perm[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { ev[k] = A[k][k]; perm[k] = k; }
    for (int i = 1; i < 6; ++i) { // stable: an eigenvalue moves left only past strictly larger ones
        const int pi = perm[i];
        int j = i;
        while (j > 0 && ev[pi] < ev[perm[j - 1]]) { perm[j] = perm[j - 1]; --j; }
        perm[j] = pi;
    }
    for (int k = 0; k < 6; ++k) {
        const int pk = perm[k];
        d->info.eigval[k] = ev[pk];
        for (int j = 0; j < 6; ++j) {
            double x = 0.0;
#pragma unroll
            for (int jj = 0; jj < 6; ++jj) x = jj == pk ? V[j][jj] : x;
            d->info.basis[6 * k + j] = x;
        }
    }
}

// per point: the weights (v . x_k)^2 of the six directions, and the sort pairs of lists k0 .. k0 + g - 1:
// key (k - k0) << 32 | ~bits((float)|v . x_k|), value = the point's index
__global__ __launch_bounds__(CB) void cs_key_kernel(const float4* __restrict__ pts, const float* __restrict__ nrm, int64_t n, const CsDev* __restrict__ d,
                                                    int k0, int g, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                    double* __restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * CB + threadIdx.x;
    if (i >= n) return;
    const double c[3] = {d->info.center[0], d->info.center[1], d->info.center[2]};
    const double s = 1.0 / d->info.lnorm;
    double v[6];
    cs_vec(pts[i], nrm, i, c, s, v);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double* x = d->info.basis + 6 * k;
        double m = v[0] * x[0];
#pragma unroll
        for (int j = 1; j < 6; ++j) m = m + v[j] * x[j];
        w[6 * i + k] = m * m;
        if (k >= k0 && k < k0 + g) {
            const unsigned bits = __float_as_uint((float)fabs(m));
            const size_t e = (size_t)(k - k0) * (size_t)n + (size_t)i;
            keys[e] = ((unsigned long long)(k - k0) << 32) | (unsigned long long)(~bits);
            vals[e] = (unsigned)i;
        }
    }
}

// six per-list values in named registers: get / set at a wave-uniform list index are select chains (an array indexed that way, even
// through unrolled selects, was folded back into a dynamic index and kept in private memory)
template <typename T>
struct CsSix {
    T a0, a1, a2, a3, a4, a5;
    __device__ __forceinline__ T get(int k) const { return k == 0 ? a0 : k == 1 ? a1 : k == 2 ? a2 : k == 3 ? a3 : k == 4 ? a4 : a5; }
    __device__ __forceinline__ void set(int k, T v)
    {
        a0 = k == 0 ? v : a0; a1 = k == 1 ? v : a1; a2 = k == 2 ? v : a2;
        a3 = k == 3 ? v : a3; a4 = k == 4 ? v : a4; a5 = k == 5 ? v : a5;
    }
};

// The greedy loop, one wave.  Every list has a window: lane l holds entry base_k + l of list k (its point index in a register, its six
// weights in LDS), and a 64-bit mask of the window entries not yet selected.  A step: k = the first argmin of t; the first set bit of
// mask_k is the front of list k (everything before it is selected); the pick's weights come from LDS; six ballots clear the pick from
// every window that holds it.  Only a window that runs empty reads global memory: the next 64 list entries, their weights, and the
// selected flags of those points (LDS bitmap up to CS_LDS_POINTS, else a global bitmap written with device-scope atomics).
template <bool LDS_FLAGS>
__global__ __launch_bounds__(CS_W) void cs_greedy_kernel(const unsigned* __restrict__ lists, int64_t n, const double* __restrict__ w, int64_t nb,
                                                         unsigned* __restrict__ gbits, int* __restrict__ order, CsDev* __restrict__ d)
{
    __shared__ double sw[6][CS_W][6];
    __shared__ unsigned sbits[LDS_FLAGS ? CS_LDS_POINTS / 32 : 1];
    const int lane = threadIdx.x;
    if (LDS_FLAGS)
        for (int64_t q = lane; q < (n + 31) / 32; q += CS_W) sbits[q] = 0u;
    __syncthreads();
    CsSix<unsigned> idx = {0u, 0u, 0u, 0u, 0u, 0u};
    CsSix<unsigned long long> mask = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    CsSix<int64_t> base = {-CS_W, -CS_W, -CS_W, -CS_W, -CS_W, -CS_W};
    CsSix<double> t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int mine = 0;
    for (int64_t s = 0; s < nb; ++s) {
        int k = 0;
        double tk = t.a0;
#pragma unroll
        for (int j = 1; j < 6; ++j)
            if (t.get(j) < tk) { tk = t.get(j); k = j; }
        k = __builtin_amdgcn_readfirstlane(k);
        unsigned long long mk = mask.get(k);
        while (mk == 0ull) { // refill list k's window
            __syncthreads();
            if (!LDS_FLAGS) __threadfence(); // the picks' atomics are visible device-wide before their flags are read back
            const int64_t b = base.get(k) + CS_W;
            if (b >= n) { if (lane == 0) d->exhausted = 1; return; }
            const int64_t pos = b + lane;
            unsigned id = 0u;
            bool alive = false;
            if (pos < n) {
                id = lists[(size_t)k * (size_t)n + (size_t)pos];
                const unsigned word = LDS_FLAGS ? sbits[id >> 5] : __hip_atomic_load(gbits + (id >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                alive = ((word >> (id & 31u)) & 1u) == 0u;
                const double* src = w + 6 * (size_t)id;
#pragma unroll
                for (int j = 0; j < 6; ++j) sw[k][lane][j] = src[j];
            }
            mk = __ballot(alive);
            base.set(k, b); idx.set(k, id); mask.set(k, mk);
            __syncthreads();
        }
        const int f = __ffsll((long long)mk) - 1;
        const unsigned sel = (unsigned)__builtin_amdgcn_readlane((int)idx.get(k), f);
        if (lane == 0) {
            if (LDS_FLAGS) sbits[sel >> 5] |= 1u << (sel & 31u);
            else __hip_atomic_fetch_or(gbits + (sel >> 5), 1u << (sel & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const double* ws = sw[k][f];
        t.a0 = t.a0 + ws[0]; t.a1 = t.a1 + ws[1]; t.a2 = t.a2 + ws[2];
        t.a3 = t.a3 + ws[3]; t.a4 = t.a4 + ws[4]; t.a5 = t.a5 + ws[5];
        mask.a0 &= ~__ballot(idx.a0 == sel); mask.a1 &= ~__ballot(idx.a1 == sel); mask.a2 &= ~__ballot(idx.a2 == sel);
        mask.a3 &= ~__ballot(idx.a3 == sel); mask.a4 &= ~__ballot(idx.a4 == sel); mask.a5 &= ~__ballot(idx.a5 == sel);
        const int slot = (int)(s & (CS_W - 1));
        if (lane == slot) mine = (int)sel;
        if (slot == CS_W - 1 || s == nb - 1)
            if (lane <= slot) order[s - slot + lane] = mine;
    }
}

} // namespace

icpmi_status ops_covariance_sampling(icpmi_ctx* c, const float* in4, int64_t n, const float* normals3, int64_t nb, int torque_norm, int32_t* order_out,
                                     icpmi_covsamp_info* info_out)
{
    const int blocks = (int)((n + CB - 1) / CB);
    const int rb = blocks < CS_MAX_PARTS ? blocks : CS_MAX_PARTS;
    // lists sorted together: as many as keep g n below 2^31 (the sort's positions are 32-bit); all six for n < 357 M
    const int64_t gmax = 0x7fffffffll / n;
    const int g = gmax < 6 ? (int)gmax : 6;
    const int64_t ng = (int64_t)g * n;
    DevBuf<float4> d_in; DevBuf<float> d_nrm; DevBuf<int> d_order; DevBuf<unsigned> d_lists;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_nrm.alloc((size_t)3 * n));
    HIP_TRY(c, d_order.alloc((size_t)(nb > 0 ? nb : 1)));
    if (g < 6) HIP_TRY(c, d_lists.alloc((size_t)6 * n));
    unsigned long long* d_keys = scratch_get<unsigned long long>(c, 0, (size_t)2 * ng + 2);
    unsigned* d_vals = scratch_get<unsigned>(c, 1, (size_t)2 * ng + 2);
    unsigned* d_tab = scratch_get<unsigned>(c, 2, radix_sort_tab_words(ng, 35));
    const size_t dev_words = (sizeof(CsDev) + sizeof(double) - 1) / sizeof(double);
    double* d_part = scratch_get<double>(c, 3, (size_t)32 * rb + dev_words + 8);
    double* d_w = scratch_get<double>(c, 4, (size_t)6 * n);
    const bool lds_flags = n <= CS_LDS_POINTS;
    unsigned* d_gbits = lds_flags ? nullptr : scratch_get<unsigned>(c, 5, (size_t)(n + 31) / 32);
    if (!d_keys || !d_vals || !d_tab || !d_part || !d_w || (!lds_flags && !d_gbits)) return ICPMI_ERR_HIP;
    double* p_mom = d_part;            // 10 per workgroup
    double* p_dist = d_part + 10 * rb; // 1 per workgroup
    double* p_cov = d_part + 11 * rb;  // 21 per workgroup
    CsDev* d_dev = reinterpret_cast<CsDev*>(d_part + 32 * rb);

    HIP_TRY(c, hipMemcpyAsync(d_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_nrm, normals3, (size_t)3 * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (!lds_flags) HIP_TRY(c, hipMemsetAsync(d_gbits, 0, (size_t)(n + 31) / 32 * sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(cs_moments_kernel, dim3(rb), dim3(CB), 0, c->stream, (const float4*)d_in, (const float*)d_nrm, n, p_mom);
    hipLaunchKernelGGL(cs_center_kernel, dim3(1), dim3(CB), 0, c->stream, (const double*)p_mom, rb, n, d_dev);
    if (torque_norm == 1) hipLaunchKernelGGL(cs_dist_kernel, dim3(rb), dim3(CB), 0, c->stream, (const float4*)d_in, n, (const CsDev*)d_dev, p_dist);
    hipLaunchKernelGGL(cs_lnorm_kernel, dim3(1), dim3(CB), 0, c->stream, (const double*)p_dist, torque_norm == 1 ? rb : 0, n, torque_norm, d_dev);
    hipLaunchKernelGGL(cs_cov_kernel, dim3(rb), dim3(CB), 0, c->stream, (const float4*)d_in, (const float*)d_nrm, n, (const CsDev*)d_dev, p_cov);
    hipLaunchKernelGGL(cs_eigen_kernel, dim3(1), dim3(CB), 0, c->stream, (const double*)p_cov, rb, d_dev);
    HIP_TRY(c, hipGetLastError());
    const unsigned* lists = nullptr;
    for (int k0 = 0; k0 < 6; k0 += g) {
        const int gk = 6 - k0 < g ? 6 - k0 : g;
        hipLaunchKernelGGL(cs_key_kernel, dim3(blocks), dim3(CB), 0, c->stream, (const float4*)d_in, (const float*)d_nrm, n, (const CsDev*)d_dev, k0, gk,
                           d_keys, d_vals, d_w);
        HIP_TRY(c, hipGetLastError());
        int half = 0;
        const int64_t m = (int64_t)gk * n;
        const icpmi_status s = radix_sort_pairs(c, d_keys, d_vals, m, 35, d_tab, &half);
        if (s != ICPMI_OK) return s;
        // radix_sort_pairs' halves are [0, m) and [m, 2 m) of the arrays
        const unsigned* sorted = d_vals + (half ? m : 0);
        if (g == 6) lists = sorted;
        else HIP_TRY(c, hipMemcpyAsync(d_lists.get() + (size_t)k0 * n, sorted, (size_t)m * sizeof(unsigned), hipMemcpyDeviceToDevice, c->stream));
    }
    if (g < 6) lists = d_lists;
    if (nb > 0) {
        if (lds_flags)
            hipLaunchKernelGGL(cs_greedy_kernel<true>, dim3(1), dim3(CS_W), 0, c->stream, lists, n, (const double*)d_w, nb, (unsigned*)nullptr,
                               (int*)d_order, d_dev);
        else
            hipLaunchKernelGGL(cs_greedy_kernel<false>, dim3(1), dim3(CS_W), 0, c->stream, lists, n, (const double*)d_w, nb, d_gbits, (int*)d_order,
                               d_dev);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(order_out, d_order, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    CsDev h;
    if (read_back(c, &h, d_dev, sizeof h) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (h.nonfinite) { c->last_error = "covariance_sampling: the cloud has non-finite coordinates or normals"; return ICPMI_ERR_INVALID_ARG; }
    if (h.exhausted) { c->last_error = "covariance_sampling: a sorted list ran out of unselected points"; return ICPMI_ERR_HIP; }
    if (info_out) *info_out = h.info;
    return ICPMI_OK;
}
