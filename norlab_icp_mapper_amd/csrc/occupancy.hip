// occupancy.hip -- global localisation: branch and bound over voxel occupancy levels (include/icpmi.h states the quantity.
// The 3D-BBS formulation of Aoki, Koide, Oishi, Yokozuka, Banno, ICRA 2024).
//   the pyramid of the resident map:  level 0: key kernel -> radix_sort_pairs (63 bits) -> head flags + scan -> the unique keys ascending;
//                                     level l >= 1 from level 0's unique keys: shift, sort, unique (occC_l), then the eight w - e, sort,
//                                     unique (occB_l); per level an open-addressing table of key-only slots (one CAS per key)
//   the node scores:                  occ_score_kernel: a workgroup keeps a slice of the reading in registers and walks a tile of nodes; a
//                                     point is rotated once per run of nodes of one rotation, a node costs a shift, an add and a probe
//   the search:                       occ_global_localize, best-first over a host heap, one launch and one read-back per round
// Integers only behind the key: any order of additions gives the same bits, and so do two runs.
#include "common.h"
#include <algorithm>
#include <chrono>
#include <vector>

namespace {

constexpr int OCC_RANGE = 1 << 19;               // |cell| < 2^19 on every axis: cell + offset stays inside the key's 21-bit fields
constexpr int OCC_PPT = 4;                       // points a thread keeps
constexpr int OCC_SLICE = 256 * OCC_PPT;         // points of a workgroup
constexpr int OCC_TILE = 16;                     // nodes a workgroup walks
constexpr int OCC_LAUNCH_NODES = 65536;          // nodes one launch carries (grid.y = 4096 tiles)

__host__ __device__ __forceinline__ unsigned long long occ_pack(int ix, int iy, int iz)
{
    return ((unsigned long long)(ix + VOX_BIAS) << 42) | ((unsigned long long)(iy + VOX_BIAS) << 21) | (unsigned long long)(iz + VOX_BIAS);
}
__host__ __device__ __forceinline__ void occ_unpack(unsigned long long key, int* ix, int* iy, int* iz)
{
    *ix = (int)((key >> 42) & 0x1fffff) - VOX_BIAS; *iy = (int)((key >> 21) & 0x1fffff) - VOX_BIAS; *iz = (int)(key & 0x1fffff) - VOX_BIAS;
}

// ---- the pyramid ----------------------------------------------------------------------------------
// level 0's keys: vox_key's packing with the narrower range; a point out of it raises `bad`
__global__ __launch_bounds__(256) void occ_key_kernel(const float4* __restrict__ pts, int64_t m, float s0, unsigned long long* __restrict__ keys,
                                                      unsigned* __restrict__ vals, unsigned* __restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float4 p = pts[i];
    unsigned long long k = 0;
    bool ok = vox_key(p.x, p.y, p.z, s0, &k);
    if (ok) {
        int ix, iy, iz;
        occ_unpack(k, &ix, &iy, &iz);
        ok = ix > -OCC_RANGE && ix < OCC_RANGE && iy > -OCC_RANGE && iy < OCC_RANGE && iz > -OCC_RANGE && iz < OCC_RANGE;
    }
    if (!ok) { atomicOr(bad, 1u); k = 0; }
    keys[i] = k;
    vals[i] = (unsigned)i;
}

// occC_l's members, with repeats: every field of a level-0 key shifted arithmetically
__global__ __launch_bounds__(256) void occ_shift_kernel(const unsigned long long* __restrict__ k0, int64_t nk, int l, unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nk) return;
    int ix, iy, iz;
    occ_unpack(k0[i], &ix, &iy, &iz);
    keys[i] = occ_pack(ix >> l, iy >> l, iz >> l);
    vals[i] = (unsigned)i;
}

// occB_l's members, with repeats: w - e for the eight e of {0, 1}^3
__global__ __launch_bounds__(256) void occ_expand_kernel(const unsigned long long* __restrict__ kc, int64_t nc, unsigned long long* __restrict__ keys,
                                                         unsigned* __restrict__ vals)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 8 * nc) return;
    int ix, iy, iz;
    occ_unpack(kc[i >> 3], &ix, &iy, &iz);
    const int e = (int)(i & 7);
    keys[i] = occ_pack(ix - ((e >> 2) & 1), iy - ((e >> 1) & 1), iz - (e & 1));
    vals[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void occ_head_kernel(const unsigned long long* __restrict__ skeys, int64_t n, unsigned* __restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) head[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void occ_compact_kernel(const unsigned long long* __restrict__ skeys, const unsigned* __restrict__ head,
                                                          const unsigned* __restrict__ pos, int64_t n, unsigned long long* __restrict__ ukeys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && head[i]) ukeys[pos[i]] = skeys[i];
}

// one compare-and-swap per key claims a slot; which slot a key lands in may depend on arrival order, what a probe answers may not
__global__ __launch_bounds__(256) void occ_fill_kernel(const unsigned long long* __restrict__ ukeys, int64_t nk, unsigned long long* __restrict__ tab,
                                                       unsigned mask)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nk) return;
    const unsigned long long key = ukeys[v];
    unsigned slot = vox_hash(key, mask);
    for (unsigned step = 0; step <= mask; ++step) {
        if (atomicCAS(tab + slot, VOX_EMPTY, key) == VOX_EMPTY) return;
        slot = (slot + 1) & mask;
    }
}

// the extent of occ0 (ext: lo.x lo.y lo.z hi.x hi.y hi.z, initialised to +-2^20 by the host)
__global__ __launch_bounds__(256) void occ_extent_kernel(const unsigned long long* __restrict__ ukeys, int64_t nk, int* __restrict__ ext)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nk) return;
    int c[3];
    occ_unpack(ukeys[i], &c[0], &c[1], &c[2]);
    for (int j = 0; j < 3; ++j) { atomicMin(ext + j, c[j]); atomicMax(ext + 3 + j, c[j]); }
}

// ---- the node scores ------------------------------------------------------------------------------
// what the kernel reads of the pyramid: for every value of a node's level word a real table (the slots behind the last level repeat it)
struct OccDesc { const unsigned long long* tab[ICPMI_MAX_OCC_LEVELS]; unsigned mask[ICPMI_MAX_OCC_LEVELS]; };

__device__ __forceinline__ bool occ_probe(const unsigned long long* __restrict__ tab, unsigned mask, unsigned long long key)
{
    unsigned slot = vox_hash(key, mask);
    // (load factor <= 1/2: an empty slot ends every sequence; the bound is belt and braces against a table that is not what the host says)
    for (unsigned step = 0; step <= mask; ++step) {
        const unsigned long long k = tab[slot];
        if (k == key) return true;
        if (k == VOX_EMPTY) return false;
        slot = (slot + 1) & mask;
    }
    return false;
}

// grid = (slices of the reading, tiles of nodes).  Thread t keeps the points t, t + 256, ... of its slice.  nodes5: (k, l, A.x, A.y, A.z) per
// node, uniform over the workgroup; the host hands them over sorted by (k, l), so a tile mostly stays with one rotation and a point's cell
// is formed once per run of nodes that share k.  counts[q] (cleared by the host) receives one integer atomic add per wave and node.
// No lane past the reading forms an address of it, no node past the array is read; a rotation index outside [0, n_rot) scores 0, the
// level word is masked to a slot of `d`.
__global__ __launch_bounds__(256) void occ_score_kernel(const float4* __restrict__ reading, int n, const float* __restrict__ R9, int n_rot, float s0,
                                                        const int* __restrict__ nodes5, int n_nodes, OccDesc d, unsigned* __restrict__ counts)
{
    const int64_t e0 = (int64_t)blockIdx.x * OCC_SLICE + threadIdx.x;
    float4 pt[OCC_PPT];
#pragma unroll
    for (int u = 0; u < OCC_PPT; ++u) {
        const int64_t e = e0 + u * 256;
        pt[u] = e < n ? reading[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int cx[OCC_PPT], cy[OCC_PPT], cz[OCC_PPT];
    bool in[OCC_PPT];
#pragma unroll
    for (int u = 0; u < OCC_PPT; ++u) { cx[u] = cy[u] = cz[u] = 0; in[u] = false; }
    int cur_k = -1;
    const int q0 = (int)blockIdx.y * OCC_TILE;
    const int q1 = q0 + OCC_TILE < n_nodes ? q0 + OCC_TILE : n_nodes;
    for (int q = q0; q < q1; ++q) {
        const int* __restrict__ nd = nodes5 + 5 * (size_t)q;
        const int k = nd[0], l = nd[1] & (ICPMI_MAX_OCC_LEVELS - 1), ax = nd[2], ay = nd[3], az = nd[4];
        if (k < 0 || k >= n_rot) continue; // (uniform)
        if (k != cur_k) {
            const float* __restrict__ R = R9 + 9 * (size_t)k; // column-major: R[r][c] = R[3 c + r]
#pragma unroll
            for (int u = 0; u < OCC_PPT; ++u) {
                const float4 p = pt[u];
                const float fx = floorf(fmaf(R[6], p.z, fmaf(R[3], p.y, R[0] * p.x)) / s0);
                const float fy = floorf(fmaf(R[7], p.z, fmaf(R[4], p.y, R[1] * p.x)) / s0);
                const float fz = floorf(fmaf(R[8], p.z, fmaf(R[5], p.y, R[2] * p.x)) / s0);
                const bool ok = fabsf(fx) < (float)OCC_RANGE && fabsf(fy) < (float)OCC_RANGE && fabsf(fz) < (float)OCC_RANGE; // (NaN fails)
                in[u] = ok && e0 + u * 256 < n;
                cx[u] = ok ? (int)fx : 0; cy[u] = ok ? (int)fy : 0; cz[u] = ok ? (int)fz : 0;
            }
            cur_k = k;
        }
        const unsigned long long* __restrict__ tab = d.tab[l];
        const unsigned mask = d.mask[l];
        // (|c >> l| <= 2^19 and |A| < 2^19, checked by the host: the sum stays inside a field; the test below is for a node that is not)
        unsigned cnt = 0;
#pragma unroll
        for (int u = 0; u < OCC_PPT; ++u) {
            const int kx = (cx[u] >> l) + ax, ky = (cy[u] >> l) + ay, kz = (cz[u] >> l) + az;
            const bool fits = kx > -VOX_BIAS && kx < VOX_BIAS && ky > -VOX_BIAS && ky < VOX_BIAS && kz > -VOX_BIAS && kz < VOX_BIAS;
            const bool hit = in[u] && fits && occ_probe(tab, mask, occ_pack(kx, ky, kz));
            cnt += (unsigned)__popcll(__ballot(hit)); // (wave-uniform: the whole wave is here)
        }
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(counts + q, cnt);
    }
}

// the points that take part under one rotation (the result's `points`)
__global__ __launch_bounds__(256) void occ_points_kernel(const float4* __restrict__ reading, int n, const float* __restrict__ R, float s0,
                                                         unsigned* __restrict__ count)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool ok = false;
    if (e < n) {
        const float4 p = reading[e];
        const float fx = floorf(fmaf(R[6], p.z, fmaf(R[3], p.y, R[0] * p.x)) / s0);
        const float fy = floorf(fmaf(R[7], p.z, fmaf(R[4], p.y, R[1] * p.x)) / s0);
        const float fz = floorf(fmaf(R[8], p.z, fmaf(R[5], p.y, R[2] * p.x)) / s0);
        ok = fabsf(fx) < (float)OCC_RANGE && fabsf(fy) < (float)OCC_RANGE && fabsf(fz) < (float)OCC_RANGE;
    }
    const unsigned c = (unsigned)__popcll(__ballot(ok));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// the levels of the handle's pyramid that are those of the resident map at s0 (0: none)
int occ_levels_current(const icpmi_ctx* c, float s0)
{
    const OccPyramid& p = c->occ;
    return (p.ready && p.s0 == s0 && p.map_version == c->map_version && p.epoch == c->map_epoch) ? p.levels : 0;
}

// n keys (with repeats) in the first half of d_keys -> their distinct values ascending in `out`, *nu of them.  One stream wait (the count).
icpmi_status occ_sort_unique(icpmi_ctx* c, unsigned long long* d_keys, unsigned* d_vals, unsigned* d_tab, unsigned* d_flag, int64_t n,
                             DevArr<unsigned long long>& out, int64_t* nu)
{
    const int blocks = (int)((n + 255) / 256);
    int half = 0;
    { const icpmi_status s = radix_sort_pairs(c, d_keys, d_vals, n, 63, d_tab, &half); if (s != ICPMI_OK) return s; }
    const unsigned long long* skeys = d_keys + (half ? n : 0);
    unsigned* d_head = d_flag; unsigned* d_pos = d_flag + (n + 2); // (the scan writes out[n] behind its output)
    hipLaunchKernelGGL(occ_head_kernel, dim3(blocks), dim3(256), 0, c->stream, skeys, n, d_head);
    HIP_TRY(c, hipGetLastError());
    { const icpmi_status s = device_scan_flags_count(c, d_head, d_pos, (int)n, nu); if (s != ICPMI_OK) return s; }
    if (*nu <= 0 || *nu > n) { c->last_error = "occupancy pyramid: bad key count"; return ICPMI_ERR_HIP; }
    if (out.ensure(c, (size_t)*nu) != ICPMI_OK) return ICPMI_ERR_HIP;
    hipLaunchKernelGGL(occ_compact_kernel, dim3(blocks), dim3(256), 0, c->stream, skeys, (const unsigned*)d_head, (const unsigned*)d_pos, n, out.get());
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// the operator scratch of one sort over n keys (slots 0, 1, 2, 4, as the voxel table's build takes them)
icpmi_status occ_scratch(icpmi_ctx* c, int64_t n, unsigned long long** keys, unsigned** vals, unsigned** tab, unsigned** flag)
{
    *keys = scratch_get<unsigned long long>(c, 0, (size_t)2 * n + 2);
    *vals = scratch_get<unsigned>(c, 1, (size_t)2 * n + 2);
    *tab = scratch_get<unsigned>(c, 2, radix_sort_tab_words(n, 63));
    *flag = scratch_get<unsigned>(c, 4, (size_t)2 * (n + 2) + 8);
    return (*keys && *vals && *tab && *flag) ? ICPMI_OK : ICPMI_ERR_HIP;
}

OccDesc occ_desc(const icpmi_ctx* c)
{
    OccDesc d;
    for (int l = 0; l < ICPMI_MAX_OCC_LEVELS; ++l) { // (the slots behind the last level repeat it: whatever the level word holds, the kernel probes a real table)
        const OccLevel& lv = c->occ.lv[l < c->occ.levels ? l : c->occ.levels - 1];
        d.tab[l] = lv.tab.get(); d.mask[l] = lv.mask;
    }
    return d;
}

// One scoring launch over at most OCC_LAUNCH_NODES nodes (host, 5 ints each): upload, clear, launch, one read-back.  d_pts: the reading,
// d_R: the rotations on the device.  Scratch slots 10 and 11.
icpmi_status occ_launch(icpmi_ctx* c, const float4* d_pts, int64_t n, const float* d_R, int n_rot, const int32_t* nodes5, int n_nodes, unsigned* counts)
{
    int* d_nodes = scratch_get<int>(c, 10, (size_t)5 * n_nodes);
    unsigned* d_cnt = scratch_get<unsigned>(c, 11, (size_t)n_nodes);
    if (!d_nodes || !d_cnt) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(d_nodes, nodes5, (size_t)5 * n_nodes * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_cnt, 0, (size_t)n_nodes * sizeof(unsigned), c->stream));
    const int slices = (int)((n + OCC_SLICE - 1) / OCC_SLICE), tiles = (n_nodes + OCC_TILE - 1) / OCC_TILE;
    hipLaunchKernelGGL(occ_score_kernel, dim3(slices, tiles), dim3(256), 0, c->stream, d_pts, (int)n, d_R, n_rot, c->occ.s0, (const int*)d_nodes, n_nodes,
                       occ_desc(c), d_cnt);
    HIP_TRY(c, hipGetLastError());
    return read_back(c, counts, d_cnt, (size_t)n_nodes * sizeof(unsigned)); // (waits: nodes5 is the caller's until here)
}

icpmi_status occ_upload_rotations(icpmi_ctx* c, const float* R9, int n_rot, const float** d_R)
{
    float* d = scratch_get<float>(c, 12, (size_t)9 * n_rot);
    if (!d) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(d, R9, (size_t)9 * n_rot * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (R9 is the caller's)
    *d_R = d;
    return ICPMI_OK;
}

struct OccNode { int k, l, a[3]; };
struct OccEntry { int64_t bound; OccNode q; };
// the heap's order: bound descending, level ascending, k ascending, A lexicographic
bool occ_before(const OccEntry& x, const OccEntry& y)
{
    if (x.bound != y.bound) return x.bound > y.bound;
    if (x.q.l != y.q.l) return x.q.l < y.q.l;
    if (x.q.k != y.q.k) return x.q.k < y.q.k;
    for (int j = 0; j < 3; ++j) if (x.q.a[j] != y.q.a[j]) return x.q.a[j] < y.q.a[j];
    return false;
}

} // namespace

void occ_shape(int32_t* slice, int32_t* tile, int32_t* launch_nodes) { *slice = OCC_SLICE; *tile = OCC_TILE; *launch_nodes = OCC_LAUNCH_NODES; }

// Builds the levels 0 .. levels - 1 of the resident map's pyramid at s0 that the handle does not hold: a level is a function of (map, s0, l)
// alone, so a pyramid of fewer levels is extended and one of more serves as it is.  Stream-ordered but for the counts' waits.
icpmi_status occ_ensure(icpmi_ctx* c, float s0, int levels)
{
    const int have = occ_levels_current(c, s0);
    if (have >= levels) return ICPMI_OK;
    OccPyramid& p = c->occ;
    p.ready = false;
    const int64_t m = c->m;
    if (m > 0x0fffffff) { c->last_error = "occupancy pyramid: too many map points"; return ICPMI_ERR_UNSUPPORTED; }
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t) { return std::chrono::duration<float, std::milli>(clk::now() - t).count(); };
    unsigned long long* d_keys; unsigned* d_vals; unsigned* d_tab; unsigned* d_flag;
    auto fill = [&](OccLevel& lv) -> icpmi_status {
        unsigned cap = 2;
        while ((uint64_t)cap < 2 * (uint64_t)lv.nk) cap <<= 1;
        if (lv.tab.ensure(c, (size_t)cap) != ICPMI_OK) return ICPMI_ERR_HIP;
        HIP_TRY(c, hipMemsetAsync(lv.tab.get(), 0xff, (size_t)cap * sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(occ_fill_kernel, dim3((int)((lv.nk + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)lv.keys.get(), lv.nk,
                           lv.tab.get(), cap - 1);
        HIP_TRY(c, hipGetLastError());
        lv.mask = cap - 1;
        return ICPMI_OK;
    };
    if (have == 0) { // level 0: the cells of the map's points
        const clk::time_point t0 = clk::now();
        if (occ_scratch(c, m, &d_keys, &d_vals, &d_tab, &d_flag) != ICPMI_OK) return ICPMI_ERR_HIP;
        unsigned* d_bad = d_flag + 2 * (m + 2);
        int* d_ext = (int*)(d_bad + 1);
        const int ext0[6] = {VOX_BIAS, VOX_BIAS, VOX_BIAS, -VOX_BIAS, -VOX_BIAS, -VOX_BIAS};
        HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned), c->stream));
        { const icpmi_status s = upload_small(c, d_ext, ext0, sizeof ext0); if (s != ICPMI_OK) return s; }
        hipLaunchKernelGGL(occ_key_kernel, dim3((int)((m + 255) / 256)), dim3(256), 0, c->stream, (const float4*)c->d_map_sorted, m, s0, d_keys, d_vals, d_bad);
        HIP_TRY(c, hipGetLastError());
        { const icpmi_status s = occ_sort_unique(c, d_keys, d_vals, d_tab, d_flag, m, p.lv[0].keys, &p.lv[0].nk); if (s != ICPMI_OK) return s; }
        hipLaunchKernelGGL(occ_extent_kernel, dim3((int)((p.lv[0].nk + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)p.lv[0].keys.get(),
                           p.lv[0].nk, d_ext);
        HIP_TRY(c, hipGetLastError());
        unsigned back[7] = {0};
        if (read_back(c, back, d_bad, sizeof back) != ICPMI_OK) return ICPMI_ERR_HIP;
        if (back[0]) {
            c->last_error = "global localize: a map point has a non-finite coordinate or lies 2^19 or more cells from the map's centroid on one axis";
            return ICPMI_ERR_INVALID_ARG;
        }
        for (int j = 0; j < 3; ++j) { p.cell_lo[j] = (int)back[1 + j]; p.cell_hi[j] = (int)back[4 + j]; }
        { const icpmi_status s = fill(p.lv[0]); if (s != ICPMI_OK) return s; }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        p.lv[0].build_ms = ms_since(t0);
    }
    DevBuf<unsigned long long> occC;
    for (int l = have > 1 ? have : 1; l < levels; ++l) {
        const clk::time_point t0 = clk::now();
        const int64_t n0 = p.lv[0].nk;
        if (occ_scratch(c, n0, &d_keys, &d_vals, &d_tab, &d_flag) != ICPMI_OK) return ICPMI_ERR_HIP;
        hipLaunchKernelGGL(occ_shift_kernel, dim3((int)((n0 + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)p.lv[0].keys.get(), n0, l,
                           d_keys, d_vals);
        HIP_TRY(c, hipGetLastError());
        int64_t nc = 0;
        { const icpmi_status s = occ_sort_unique(c, d_keys, d_vals, d_tab, d_flag, n0, occC, &nc); if (s != ICPMI_OK) return s; }
        const int64_t n8 = 8 * nc;
        if (occ_scratch(c, n8, &d_keys, &d_vals, &d_tab, &d_flag) != ICPMI_OK) return ICPMI_ERR_HIP;
        hipLaunchKernelGGL(occ_expand_kernel, dim3((int)((n8 + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)occC.get(), nc, d_keys, d_vals);
        HIP_TRY(c, hipGetLastError());
        { const icpmi_status s = occ_sort_unique(c, d_keys, d_vals, d_tab, d_flag, n8, p.lv[l].keys, &p.lv[l].nk); if (s != ICPMI_OK) return s; }
        { const icpmi_status s = fill(p.lv[l]); if (s != ICPMI_OK) return s; }
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        p.lv[l].build_ms = ms_since(t0);
    }
    for (int l = levels; l < ICPMI_MAX_OCC_LEVELS; ++l) { p.lv[l].nk = 0; p.lv[l].mask = 0; p.lv[l].build_ms = 0.f; }
    p.levels = levels; p.s0 = s0; p.map_version = c->map_version; p.epoch = c->map_epoch;
    if (have == 0) ++p.builds;
    p.ready = true;
    return ICPMI_OK;
}

icpmi_status occ_get_level(icpmi_ctx* c, float s0, int levels, int level, int64_t cap, int32_t* ijk3, int64_t* n_keys)
{
    { const icpmi_status s = occ_ensure(c, s0, levels); if (s != ICPMI_OK) return s; }
    const OccLevel& lv = c->occ.lv[level];
    if (n_keys) *n_keys = lv.nk;
    if (!ijk3 && cap == 0) return ICPMI_OK; // (a size query: *n_keys alone)
    if (cap < lv.nk) { c->last_error = "get_occupancy_level: capacity below the key count (*n_keys has it)"; return ICPMI_ERR_INVALID_ARG; }
    std::vector<unsigned long long> keys((size_t)lv.nk);
    HIP_TRY(c, hipMemcpyAsync(keys.data(), lv.keys.get(), (size_t)lv.nk * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (ijk3)
        for (int64_t v = 0; v < lv.nk; ++v) occ_unpack(keys[(size_t)v], ijk3 + 3 * v, ijk3 + 3 * v + 1, ijk3 + 3 * v + 2);
    return ICPMI_OK;
}

icpmi_status occ_score_nodes(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* R9, int n_rot, float s0, int levels, const int32_t* nodes5,
                             int64_t n_nodes, int64_t* counts)
{
    { const icpmi_status s = occ_ensure(c, s0, levels); if (s != ICPMI_OK) return s; }
    const float* d_R = nullptr;
    { const icpmi_status s = occ_upload_rotations(c, R9, n_rot, &d_R); if (s != ICPMI_OK) return s; }
    std::vector<unsigned> got((size_t)std::min<int64_t>(n_nodes, OCC_LAUNCH_NODES));
    for (int64_t q0 = 0; q0 < n_nodes; q0 += OCC_LAUNCH_NODES) {
        const int cnt = (int)std::min<int64_t>(OCC_LAUNCH_NODES, n_nodes - q0);
        { const icpmi_status s = occ_launch(c, d_scan, n, d_R, n_rot, nodes5 + 5 * q0, cnt, got.data()); if (s != ICPMI_OK) return s; }
        for (int i = 0; i < cnt; ++i) counts[q0 + i] = (int64_t)got[(size_t)i];
    }
    return ICPMI_OK;
}

// The search (include/icpmi.h states it).  Nodes of a launch go to the device sorted by (k, l, A): a workgroup's tile then mostly shares a
// rotation; which leaf wins and what is pushed do not depend on that order.
icpmi_status occ_global_localize(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* R9, int n_rot, float s0, int levels, const int64_t a_min[3],
                                 const int64_t a_max[3], int batch, int64_t need, int64_t max_nodes, icpmi_global_localize_result* res)
{
    { const icpmi_status s = occ_ensure(c, s0, levels); if (s != ICPMI_OK) return s; }
    const float* d_R = nullptr;
    { const icpmi_status s = occ_upload_rotations(c, R9, n_rot, &d_R); if (s != ICPMI_OK) return s; }
    const int L = levels;
    int64_t best = need - 1;
    OccNode leaf{-1, 0, {0, 0, 0}};
    std::vector<OccEntry> heap; // (std::push_heap's "less": the entry that comes later in the heap's order)
    auto later = [](const OccEntry& x, const OccEntry& y) { return occ_before(y, x); };
    std::vector<OccNode> nodes;
    std::vector<int32_t> flat;
    std::vector<unsigned> got;
    bool capped = false;
    // one launch: the scores, then the leaves in the heap's order (strictly better only), then the inner nodes onto the heap
    auto take = [&]() -> icpmi_status {
        if (nodes.empty()) return ICPMI_OK;
        std::sort(nodes.begin(), nodes.end(), [](const OccNode& x, const OccNode& y) {
            if (x.k != y.k) return x.k < y.k;
            if (x.l != y.l) return x.l < y.l;
            for (int j = 0; j < 3; ++j) if (x.a[j] != y.a[j]) return x.a[j] < y.a[j];
            return false;
        });
        const int cnt = (int)nodes.size();
        flat.resize((size_t)5 * cnt); got.resize((size_t)cnt);
        for (int i = 0; i < cnt; ++i) {
            const OccNode& q = nodes[(size_t)i];
            int32_t* f = flat.data() + 5 * (size_t)i;
            f[0] = q.k; f[1] = q.l; f[2] = q.a[0]; f[3] = q.a[1]; f[4] = q.a[2];
        }
        { const icpmi_status s = occ_launch(c, d_scan, n, d_R, n_rot, flat.data(), cnt, got.data()); if (s != ICPMI_OK) return s; }
        ++res->launches;
        res->nodes_scored += cnt;
        bool have = false;
        OccEntry top{0, {0, 0, {0, 0, 0}}};
        for (int i = 0; i < cnt; ++i) {
            if (nodes[(size_t)i].l != 0) continue;
            ++res->leaves_scored;
            const OccEntry e{(int64_t)got[(size_t)i], nodes[(size_t)i]};
            if (!have || occ_before(e, top)) { top = e; have = true; }
        }
        if (have && top.bound > best) { best = top.bound; leaf = top.q; }
        for (int i = 0; i < cnt; ++i) {
            if (nodes[(size_t)i].l == 0 || (int64_t)got[(size_t)i] <= best) continue;
            heap.push_back(OccEntry{(int64_t)got[(size_t)i], nodes[(size_t)i]});
            std::push_heap(heap.begin(), heap.end(), later);
        }
        nodes.clear();
        if (max_nodes > 0 && res->nodes_scored > max_nodes) capped = true;
        return ICPMI_OK;
    };
    int64_t t0[3], t1[3];
    for (int j = 0; j < 3; ++j) { t0[j] = a_min[j] >> (L - 1); t1[j] = a_max[j] >> (L - 1); }
    for (int k = 0; k < n_rot && !capped; ++k)
        for (int64_t x = t0[0]; x <= t1[0] && !capped; ++x)
            for (int64_t y = t0[1]; y <= t1[1] && !capped; ++y)
                for (int64_t z = t0[2]; z <= t1[2] && !capped; ++z) {
                    nodes.push_back(OccNode{k, L - 1, {(int)x, (int)y, (int)z}});
                    if ((int)nodes.size() == OCC_LAUNCH_NODES) { const icpmi_status s = take(); if (s != ICPMI_OK) return s; }
                }
    if (!capped) { const icpmi_status s = take(); if (s != ICPMI_OK) return s; }
    nodes.clear();
    while (!capped && !heap.empty() && heap.front().bound > best) {
        for (int popped = 0; popped < batch && !heap.empty() && heap.front().bound > best; ++popped) {
            std::pop_heap(heap.begin(), heap.end(), later);
            const OccNode q = heap.back().q;
            heap.pop_back();
            const int64_t w = (int64_t)1 << (q.l - 1);
            for (int e = 0; e < 8; ++e) {
                const int64_t ch[3] = {2 * (int64_t)q.a[0] + ((e >> 2) & 1), 2 * (int64_t)q.a[1] + ((e >> 1) & 1), 2 * (int64_t)q.a[2] + (e & 1)};
                bool meets = true;
                for (int j = 0; j < 3; ++j) meets = meets && ch[j] * w + w - 1 >= a_min[j] && ch[j] * w <= a_max[j];
                if (meets) nodes.push_back(OccNode{q.k, q.l - 1, {(int)ch[0], (int)ch[1], (int)ch[2]}});
            }
        }
        // (batch <= OCC_LAUNCH_NODES / 8: a round's children fit one launch)
        { const icpmi_status s = take(); if (s != ICPMI_OK) return s; }
    }
    res->proven = capped ? 0 : 1;
    res->levels = L;
    if (leaf.k < 0) return ICPMI_OK;
    res->found = 1; res->rotation = leaf.k; res->score = best;
    for (int j = 0; j < 3; ++j) res->cell[j] = leaf.a[j];
    const float* R = R9 + 9 * (size_t)leaf.k;
    for (int cc = 0; cc < 3; ++cc) for (int r = 0; r < 3; ++r) res->T[4 * cc + r] = R[3 * cc + r];
    for (int r = 0; r < 3; ++r) res->T[12 + r] = (float)((double)c->mean[r] + (double)s0 * (double)leaf.a[r]);
    unsigned* d_cnt = scratch_get<unsigned>(c, 11, 1);
    if (!d_cnt) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned), c->stream));
    hipLaunchKernelGGL(occ_points_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, d_scan, (int)n, d_R + 9 * (size_t)leaf.k, s0, d_cnt);
    HIP_TRY(c, hipGetLastError());
    unsigned pts = 0;
    if (read_back(c, &pts, d_cnt, sizeof pts) != ICPMI_OK) return ICPMI_ERR_HIP;
    res->points = (int64_t)pts;
    return ICPMI_OK;
}
