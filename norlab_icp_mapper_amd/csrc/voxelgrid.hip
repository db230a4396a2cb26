// voxelgrid.hip -- VoxelGridDataPointsFilter{vSizeX, vSizeY, vSizeZ, useCentroid: 1, averageExistingDescriptors} on the device
// (libpointmatcher DataPointsFilters/VoxelGrid.cpp, as recalled: its source is not vendored; the formulation is written down in
// include/icpmi.h next to icpmi_voxel_grid and in INTEGRATION.md).
//
// Upstream's voxel index of a point is a lattice over the bounding box, in float:
//   minB = minV / vSize, maxB = maxV / vSize, numDiv = (unsigned)((1 + maxB) - minB) per axis,
//   i = (unsigned)floor(x / vSizeX - minB.x) (j, k the same on y, z), idx = i + j numDiv.x + k numDiv.x numDiv.y (uint32).
// The points of one idx form a voxel; the voxel's output point is the centroid of its members, summed in float in index order
// starting from the first member (the smallest index), divided by the count; the output is in ascending first-member order.
// Here:
//   1. min / max / finiteness reduction (common.h: bbox_partials_kernel -> vg_grid_kernel: minB, numDiv), one small read-back for the limit checks;
//   2. idx per point (vg_key_kernel), every division correctly rounded (HIP's default for float `/`; -ffp-contract=off);
//   3. stable LSD radix sort of (idx, index) on all 32 bits (six 6-bit passes): a voxel is one run, its members in index order;
//   4. run heads -> voxel starts (scan A, stays on the device), first members flagged in index order -> output slots (scan B,
//      whose count is the one host wait that sizes the download);
//   5. the features and the averaged descriptor rows are gathered into sorted order (structure of arrays, coalesced reads next);
//   6. one lane per voxel sums its run sequentially and writes its output slot.
// No float atomics anywhere: every sum has one fixed order, and two calls give the same bits.
//
// Step 6 is a serial chain per voxel: its length is the population of the largest voxel (all points of a cloud in one 50 m voxel:
// the whole cloud on one lane).  The loads of a run are contiguous and issued 16 members x 3 rows at a time ahead of the adds; the measured cost
// of that tail is in DESIGN.md (scripts/voxel_grid_bench.py).
#include "common.h"

namespace {

constexpr int VB = 256;
static_assert(VB == BBOX_WG, "vg_grid_kernel folds the partials with bbox_fold");

struct VgGrid {
    float minB[3];
    float numDivF[3]; // (1 + maxB) - minB, before the truncation (the 2^24 limit is checked on it)
    unsigned numDiv[3];
    int nonfinite;
};

// one block: the blocks' partials -> the grid (min / max are exact, so the order of the reduction does not matter)
__global__ __launch_bounds__(VB) void vg_grid_kernel(const float* __restrict__ part, const unsigned* __restrict__ bad, int nparts, float vx, float vy,
                                                     float vz, VgGrid* __restrict__ g)
{
    float lo[3], hi[3];
    unsigned nbad;
    bbox_fold<true>(part, bad, nparts, lo, hi, nbad);
    if (threadIdx.x == 0) {
        const float vs[3] = {vx, vy, vz};
        for (int r = 0; r < 3; ++r) {
            const float minB = lo[r] / vs[r];
            const float maxB = hi[r] / vs[r];
            const float nd = (1.f + maxB) - minB;
            g->minB[r] = minB;
            g->numDivF[r] = nd;
            g->numDiv[r] = (nd >= 0.f && nd < 4294967296.f) ? (unsigned)nd : 0u; // (out-of-range values are rejected by the host)
        }
        g->nonfinite = nbad ? 1 : 0;
    }
}

__device__ __forceinline__ unsigned vg_cell(float v, float vs, float minB) { return (unsigned)floorf(v / vs - minB); }

__global__ __launch_bounds__(VB) void vg_key_kernel(const float4* __restrict__ pts, int64_t n, float vx, float vy, float vz, const VgGrid* __restrict__ g,
                                                    unsigned long long* __restrict__ keys, unsigned* __restrict__ vals)
{
    const int64_t p = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (p >= n) return;
    const float4 q = pts[p];
    const unsigned d0 = g->numDiv[0], d01 = g->numDiv[0] * g->numDiv[1];
    const unsigned idx = vg_cell(q.x, vx, g->minB[0]) + vg_cell(q.y, vy, g->minB[1]) * d0 + vg_cell(q.z, vz, g->minB[2]) * d01;
    keys[p] = (unsigned long long)idx;
    vals[p] = (unsigned)p;
}

// sorted position j: head[j] = 1 iff j starts a run of equal idx; first[vals[j]] = the same flag in index order (every index is written
// exactly once, so first[] needs no clearing)
__global__ __launch_bounds__(VB) void vg_head_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals, int64_t n,
                                                     unsigned* __restrict__ head, unsigned* __restrict__ first)
{
    const int64_t j = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (j >= n) return;
    const unsigned h = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
    head[j] = h;
    first[vals[j]] = h;
}

// vstart[v] = sorted position of the head of voxel v, vstart[#voxels] = n
__global__ __launch_bounds__(VB) void vg_start_kernel(const unsigned* __restrict__ head, const unsigned* __restrict__ vnum, int64_t n, unsigned* __restrict__ vstart)
{
    const int64_t j = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (j >= n) return;
    if (head[j]) vstart[vnum[j]] = (unsigned)j;
    if (j == n - 1) vstart[vnum[j] + head[j]] = (unsigned)n;
}

// the rows that are summed, in sorted order: rows 0..2 = x, y, z; rows 3.. = the descriptor rows (when they are averaged)
__global__ __launch_bounds__(VB) void vg_gather_kernel(const float4* __restrict__ pts, const float* __restrict__ desc, int rows, const unsigned* __restrict__ vals,
                                                       int64_t n, float* __restrict__ soa)
{
    const int64_t j = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (j >= n) return;
    const unsigned i = vals[j];
    const float4 q = pts[i];
    soa[j] = q.x; soa[n + j] = q.y; soa[2 * n + j] = q.z;
    for (int r = 0; r < rows; ++r) soa[(3 + r) * n + j] = desc[(size_t)i * rows + r];
}

// sequential float sums of R rows a[r][0 .. cnt), each starting from a[r][0]: the loads of VG_U members of every row go out ahead of
// the (ordered) adds, so a long run is bound by R * VG_U loads in flight rather than by one load latency per member
constexpr int VG_U = 16;
template <int R>
__device__ __forceinline__ void vg_run_sums(const float* const (&a)[R], unsigned cnt, float (&s)[R])
{
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = a[r][0];
    unsigned e = 1;
    for (; e + VG_U <= cnt; e += VG_U) {
        float v[R][VG_U];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < VG_U; ++u) v[r][u] = a[r][e + u];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int u = 0; u < VG_U; ++u) s[r] = s[r] + v[r][u];
    }
    for (; e < cnt; ++e)
#pragma unroll
        for (int r = 0; r < R; ++r) s[r] = s[r] + a[r][e];
}

// one lane per voxel: centroid (and averaged descriptor rows) into the output slot of its first member
__global__ __launch_bounds__(VB) void vg_sum_kernel(const float* __restrict__ soa, int64_t n, const unsigned* __restrict__ vstart, int64_t nvox,
                                                    const unsigned* __restrict__ vals, const unsigned* __restrict__ opos, const float4* __restrict__ pts,
                                                    const float* __restrict__ desc, int rows, int average, int* __restrict__ order_out,
                                                    float4* __restrict__ out4, float* __restrict__ desc_out)
{
    const int64_t v = (int64_t)blockIdx.x * VB + threadIdx.x;
    if (v >= nvox) return;
    const unsigned s0 = vstart[v], s1 = vstart[v + 1];
    if (s1 <= s0 || s1 > (unsigned)n) return; // (cannot happen: scans A and B count the same voxels)
    const unsigned cnt = s1 - s0;
    const unsigned f = vals[s0];
    const unsigned o = opos[f];
    const float fc = (float)cnt;
    const float* const xyz[3] = {soa + s0, soa + n + s0, soa + 2 * n + s0};
    float sxyz[3];
    vg_run_sums<3>(xyz, cnt, sxyz);
    float4 q;
    q.x = sxyz[0] / fc;
    q.y = sxyz[1] / fc;
    q.z = sxyz[2] / fc;
    q.w = pts[f].w; // the homogeneous row stays the first member's
    out4[o] = q;
    order_out[o] = (int)f;
    for (int r = 0; r < rows; ++r) {
        float d = desc[(size_t)f * rows + r];
        if (average) {
            const float* const row[1] = {soa + (size_t)(3 + r) * n + s0};
            float sd[1];
            vg_run_sums<1>(row, cnt, sd);
            d = sd[0] / fc;
        }
        desc_out[(size_t)o * rows + r] = d;
    }
}

} // namespace

icpmi_status ops_voxel_grid(icpmi_ctx* c, const float* in4, int64_t n, const float vsize[3], int average, const float* desc, int rows,
                            int32_t* order_out, float* out4, float* desc_out, int64_t* n_out)
{
    *n_out = 0;
    if (n == 0) return ICPMI_OK;
    const int blocks = (int)((n + VB - 1) / VB);
    const int rb = blocks < 1024 ? blocks : 1024;
    const int srows = 3 + (average ? rows : 0);
    DevBuf<float4> d_in; DevBuf<float> d_desc, d_soa, d_out4, d_dout; DevBuf<int> d_order;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_soa.alloc((size_t)srows * n));
    HIP_TRY(c, d_out4.alloc((size_t)4 * n));
    HIP_TRY(c, d_order.alloc((size_t)n));
    if (rows > 0) { HIP_TRY(c, d_desc.alloc((size_t)rows * n)); HIP_TRY(c, d_dout.alloc((size_t)rows * n)); }
    unsigned long long* d_keys = scratch_get<unsigned long long>(c, 0, (size_t)2 * n + 2);
    unsigned* d_vals = scratch_get<unsigned>(c, 1, (size_t)2 * n + 2);
    unsigned* d_tab = scratch_get<unsigned>(c, 2, radix_sort_tab_words(n, 32));
    float* d_part = scratch_get<float>(c, 3, (size_t)7 * rb + sizeof(VgGrid) / sizeof(float) + 8);
    const int64_t fs = n + 2; // the scans write out[n] (their total) behind every output array
    unsigned* d_flag = scratch_get<unsigned>(c, 4, (size_t)4 * fs + 4); // head | vnum | first | opos | scan A's total
    unsigned* d_vstart = scratch_get<unsigned>(c, 5, (size_t)n + 2);
    if (!d_keys || !d_vals || !d_tab || !d_part || !d_flag || !d_vstart) return ICPMI_ERR_HIP;
    unsigned* d_bad = reinterpret_cast<unsigned*>(d_part + 6 * rb);
    VgGrid* d_grid = reinterpret_cast<VgGrid*>(d_part + 7 * rb + 1);
    unsigned* d_head = d_flag;
    unsigned* d_vnum = d_flag + fs;
    unsigned* d_first = d_flag + 2 * fs;
    unsigned* d_opos = d_flag + 3 * fs;
    unsigned* d_nvox = d_flag + 4 * fs; // scan A's total (not read: scan B's count is the same number)

    HIP_TRY(c, hipMemcpyAsync(d_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (rows > 0) HIP_TRY(c, hipMemcpyAsync(d_desc, desc, (size_t)rows * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bbox_partials_kernel<true>, dim3(rb), dim3(BBOX_WG), 0, c->stream, (const float4*)d_in, n, d_part, d_bad, 3.402823466e38f /* FLT_MAX */);
    hipLaunchKernelGGL(vg_grid_kernel, dim3(1), dim3(VB), 0, c->stream, (const float*)d_part, (const unsigned*)d_bad, rb, vsize[0], vsize[1], vsize[2], d_grid);
    HIP_TRY(c, hipGetLastError());
    VgGrid g;
    if (read_back(c, &g, d_grid, sizeof g) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (g.nonfinite) { c->last_error = "voxel_grid: the cloud has non-finite coordinates"; return ICPMI_ERR_INVALID_ARG; }
    for (int r = 0; r < 3; ++r)
        if (!(g.numDivF[r] < 16777216.f)) {
            c->last_error = "voxel_grid: the cloud spans 2^24 or more voxels on one axis (upstream's float indices would alias)";
            return ICPMI_ERR_INVALID_ARG;
        }
    if ((unsigned long long)g.numDiv[0] * g.numDiv[1] * g.numDiv[2] > 0xffffffffull) {
        c->last_error = "voxel_grid: numDivX * numDivY * numDivZ exceeds 2^32 - 1 (upstream's 32-bit voxel index would wrap)";
        return ICPMI_ERR_INVALID_ARG;
    }

    hipLaunchKernelGGL(vg_key_kernel, dim3(blocks), dim3(VB), 0, c->stream, (const float4*)d_in, n, vsize[0], vsize[1], vsize[2], (const VgGrid*)d_grid,
                       d_keys, d_vals);
    HIP_TRY(c, hipGetLastError());
    int half = 0;
    // all 32 bits: idx stays below numDivX numDivY numDivZ except where (1 + maxB) rounds to maxB (coordinates beyond 2^24 voxel edges),
    // and the grouping must be by idx whatever its range
    {
        const icpmi_status s = radix_sort_pairs(c, d_keys, d_vals, n, 32, d_tab, &half);
        if (s != ICPMI_OK) return s;
    }
    const unsigned long long* skeys = d_keys + (half ? n : 0);
    const unsigned* svals = d_vals + (half ? n : 0);
    hipLaunchKernelGGL(vg_head_kernel, dim3(blocks), dim3(VB), 0, c->stream, skeys, svals, n, d_head, d_first);
    HIP_TRY(c, hipGetLastError());
    {
        const icpmi_status s = device_exclusive_scan_sum(c, d_head, d_vnum, (int)n, d_nvox);
        if (s != ICPMI_OK) return s;
    }
    hipLaunchKernelGGL(vg_start_kernel, dim3(blocks), dim3(VB), 0, c->stream, (const unsigned*)d_head, (const unsigned*)d_vnum, n, d_vstart);
    hipLaunchKernelGGL(vg_gather_kernel, dim3(blocks), dim3(VB), 0, c->stream, (const float4*)d_in, (const float*)d_desc, average ? rows : 0, svals, n,
                       (float*)d_soa);
    HIP_TRY(c, hipGetLastError());
    int64_t m = 0;
    {
        const icpmi_status s = device_scan_flags_count(c, d_first, d_opos, (int)n, &m);
        if (s != ICPMI_OK) return s;
    }
    if (m <= 0 || m > n) { c->last_error = "voxel_grid: bad voxel count"; return ICPMI_ERR_HIP; }
    hipLaunchKernelGGL(vg_sum_kernel, dim3((int)((m + VB - 1) / VB)), dim3(VB), 0, c->stream, (const float*)d_soa, n, (const unsigned*)d_vstart, m, svals,
                       (const unsigned*)d_opos, (const float4*)d_in, (const float*)d_desc, rows, average, (int*)d_order, (float4*)d_out4.get(),
                       (float*)d_dout);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out4, d_out4, (size_t)m * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (order_out) HIP_TRY(c, hipMemcpyAsync(order_out, d_order, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (rows > 0 && desc_out) HIP_TRY(c, hipMemcpyAsync(desc_out, d_dout, (size_t)m * rows * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_out = m;
    return ICPMI_OK;
}
