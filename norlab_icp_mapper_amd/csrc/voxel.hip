// voxel.hip -- VoxelMatcher: voxelised plane-to-plane ICP with no neighbour search (Koide et al., ICRA 2021, with one voxel
// per reading point: the "DIRECT1" neighbourhood).
//   the table of the resident map:  key kernel -> radix_sort_pairs (63 bits, stable: a voxel's members stay in ascending resident index)
//                                   -> head flags + scan -> one wave per voxel sums its run in double -> open-addressing fill (one CAS per voxel)
//   the iteration's pair sums:      voxel_pairs_kernel: one point load, one probe, the sums of DESIGN.md 4.15 with q = mu and
//                                   M = (C_v + C(u_p))^-1, into the fixed-point accumulators the existing solve kernel reads
//   a schedule of sizes (4.21):     one table per level by the same build; voxel_pairs_sched_kernel: the same pair sums with table, mask and
//                                   size taken from the level descriptors by the level the loop header holds (loop.hip raises it)
//   a batch of readings (4.23):     voxel_pairs_batch_kernel: the same pair sums with blockIdx.y = member, every member on the workgroups and
//                                   in the order of additions it has alone (loop.hip: loop_run_voxel_batch drives it)
// No float atomics anywhere: two builds of one map give the same bits, and so do two registrations.
#include "common.h"
#include <vector>

namespace {

// (the key of a centred point and where its probe sequence starts: common.h, vox_key and vox_hash -- occupancy.hip packs the same key)
// A slot of the table is one 64-byte line, read as four 16-byte words that one probe requests together:
//   [0] key lo, key hi, ordinal in ascending key order, count     [1] mu.x mu.y mu.z Nxx     [2] Nxy Nxz Nyy Nyz     [3] Nzz 0 0 0
// The sorted records (what icpmi_get_voxel_map hands out) are words [1..3] with the count in [3].y.
struct VoxHit { float4 a, b, c; int ordinal; };

__device__ __forceinline__ bool vox_probe(const uint4* __restrict__ tab, unsigned mask, unsigned long long key, VoxHit* hit)
{
    unsigned slot = vox_hash(key, mask);
    // (load factor <= 1/2: an empty slot ends every sequence; the bound is belt and braces against a table that is not what the host says)
    for (unsigned step = 0; step <= mask; ++step) {
        const uint4* s = tab + 4 * (size_t)slot;
        const uint4 w0 = s[0], w1 = s[1], w2 = s[2], w3 = s[3]; // one line, one trip
        const unsigned long long k = (unsigned long long)w0.x | ((unsigned long long)w0.y << 32);
        if (k == key) {
            hit->ordinal = (int)w0.z;
            hit->a = make_float4(__uint_as_float(w1.x), __uint_as_float(w1.y), __uint_as_float(w1.z), __uint_as_float(w1.w));
            hit->b = make_float4(__uint_as_float(w2.x), __uint_as_float(w2.y), __uint_as_float(w2.z), __uint_as_float(w2.w));
            hit->c = make_float4(__uint_as_float(w3.x), 0.f, 0.f, 0.f);
            return true;
        }
        if (k == VOX_EMPTY) return false;
        slot = (slot + 1) & mask;
    }
    return false;
}

// ---- the table ----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vox_key_kernel(const float4* __restrict__ pts, int64_t m, float size, unsigned long long* __restrict__ keys,
                                                      unsigned* __restrict__ vals, unsigned* __restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float4 p = pts[i];
    unsigned long long k = 0;
    if (!vox_key(p.x, p.y, p.z, size, &k)) atomicOr(bad, 1u);
    keys[i] = k;
    vals[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void vox_head_kernel(const unsigned long long* __restrict__ skeys, int64_t m, unsigned* __restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) head[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1u : 0u;
}

// start of every voxel's run in the sorted order; vstart[nv] = m is written by the thread of the last element
__global__ __launch_bounds__(256) void vox_start_kernel(const unsigned* __restrict__ head, const unsigned* __restrict__ pos, int64_t m,
                                                        unsigned* __restrict__ vstart)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    if (head[i]) vstart[pos[i]] = (unsigned)i;
    if (i == m - 1) vstart[pos[i] + head[i]] = (unsigned)m;
}

// One wave per voxel: lane l adds the members l, l + 64, ... of the run in that order, the 64 lane sums fold in a fixed butterfly; all in
// double, rounded once.  The order is a function of the run alone -- the same bits on every build.
__global__ __launch_bounds__(256) void vox_reduce_kernel(const unsigned long long* __restrict__ skeys, const unsigned* __restrict__ svals,
                                                         const unsigned* __restrict__ vstart, int64_t nv, const float4* __restrict__ pts,
                                                         const float4* __restrict__ normals, unsigned long long* __restrict__ ukeys,
                                                         float4* __restrict__ rec)
{
    const int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (v >= nv) return; // (wave-uniform)
    const unsigned s0 = vstart[v], s1 = vstart[v + 1];
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned i = s0 + lane; i < s1; i += 64) {
        const unsigned s = svals[i];
        const float4 p = pts[s];
        const float3 nr = *reinterpret_cast<const float3*>(normals + s);
        const float3 u = unit_or_zero(nr.x, nr.y, nr.z);
        a[0] += (double)p.x; a[1] += (double)p.y; a[2] += (double)p.z;
        a[3] += (double)u.x * (double)u.x; a[4] += (double)u.x * (double)u.y; a[5] += (double)u.x * (double)u.z;
        a[6] += (double)u.y * (double)u.y; a[7] += (double)u.y * (double)u.z; a[8] += (double)u.z * (double)u.z;
    }
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int mk = 1; mk < 64; mk <<= 1) a[j] += lane_xor_bit(a[j], mk); // (the wave is whole again behind the loop above)
    if (lane == 0) {
        const unsigned cnt = s1 - s0;
        const double inv = 1.0 / (double)cnt;
        ukeys[v] = skeys[s0];
        rec[3 * v + 0] = make_float4((float)(a[0] * inv), (float)(a[1] * inv), (float)(a[2] * inv), (float)(a[3] * inv));
        rec[3 * v + 1] = make_float4((float)(a[4] * inv), (float)(a[5] * inv), (float)(a[6] * inv), (float)(a[7] * inv));
        rec[3 * v + 2] = make_float4((float)(a[8] * inv), __uint_as_float(cnt), 0.f, 0.f);
    }
}

// one compare-and-swap per voxel claims a slot; which slot a voxel lands in may depend on arrival order, what a lookup answers may not
__global__ __launch_bounds__(256) void vox_fill_kernel(const unsigned long long* __restrict__ ukeys, const float4* __restrict__ rec, int64_t nv,
                                                       uint4* __restrict__ tab, unsigned mask)
{
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const unsigned long long key = ukeys[v];
    const float4 r0 = rec[3 * v], r1 = rec[3 * v + 1], r2 = rec[3 * v + 2];
    unsigned slot = vox_hash(key, mask);
    for (unsigned step = 0; step <= mask; ++step) {
        unsigned long long* kw = reinterpret_cast<unsigned long long*>(tab + 4 * (size_t)slot);
        if (atomicCAS(kw, VOX_EMPTY, key) == VOX_EMPTY) {
            uint4* s = tab + 4 * (size_t)slot;
            // (word 0's key half is set by the CAS: the ordinal and the count go in as two 32-bit stores behind it)
            reinterpret_cast<unsigned*>(s)[2] = (unsigned)v;
            reinterpret_cast<unsigned*>(s)[3] = __float_as_uint(r2.y);
            s[1] = make_uint4(__float_as_uint(r0.x), __float_as_uint(r0.y), __float_as_uint(r0.z), __float_as_uint(r0.w));
            s[2] = make_uint4(__float_as_uint(r1.x), __float_as_uint(r1.y), __float_as_uint(r1.z), __float_as_uint(r1.w));
            s[3] = make_uint4(__float_as_uint(r2.x), 0u, 0u, 0u);
            return;
        }
        slot = (slot + 1) & mask;
    }
}

__global__ __launch_bounds__(256) void vox_lookup_kernel(const float4* __restrict__ q, int64_t n, float size, const uint4* __restrict__ tab, unsigned mask,
                                                         int* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = q[i];
    unsigned long long key = 0;
    VoxHit hit;
    out[i] = (vox_key(p.x, p.y, p.z, size, &key) && vox_probe(tab, mask, key, &hit)) ? hit.ordinal : -1;
}

// the alternative the table was measured against (scripts/voxel_bench.py): a binary search over the sorted unique keys --
// log2(voxels) dependent loads per query where the table takes one.  Kept as a diagnostic; nothing else runs it.
__global__ __launch_bounds__(256) void vox_lookup_bsearch_kernel(const float4* __restrict__ q, int64_t n, float size,
                                                                 const unsigned long long* __restrict__ ukeys, int64_t nv, int* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = q[i];
    unsigned long long key = 0;
    int found = -1;
    if (vox_key(p.x, p.y, p.z, size, &key)) {
        int64_t lo = 0, hi = nv; // first position with ukeys[pos] >= key
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ukeys[mid] < key) lo = mid + 1; else hi = mid;
        }
        if (lo < nv && ukeys[lo] == key) found = (int)lo;
    }
    out[i] = found;
}

// ---- the pair sums ------------------------------------------------------------------------------
// Per reading point: p = T_iter x, the voxel p falls into (none: no pair), q = mu, M = (C_v + C(u_p))^-1 with C_v = I - (1 - eps) N and
// u_p = unit_or_zero(R n_x); then the sums of DESIGN.md 4.15 with weight 1 (common.h: gicp_pair_sums) and accumulate_kernel's workgroup fold
// as a function (common.h: pair_sums_fold).
// voxel_pair: one pair, the arithmetic the three pair kernels below share (g = 1 - eps; no voxel: nothing is added).
__device__ __forceinline__ void voxel_pair(const float (&T)[16], float4 r, float3 rn, const uint4* __restrict__ tab, unsigned mask, float size, float g,
                                           double (&acc)[27], double& cnt)
{
    const float3 p = xf_point(T, r.x, r.y, r.z, r.w);
    unsigned long long key = 0;
    VoxHit h;
    if (!vox_key(p.x, p.y, p.z, size, &key) || !vox_probe(tab, mask, key, &h)) return;
    cnt += 1.0;
    const float3 up = unit_or_zero(fmaf(T[8], rn.z, fmaf(T[4], rn.y, T[0] * rn.x)), fmaf(T[9], rn.z, fmaf(T[5], rn.y, T[1] * rn.x)),
                                   fmaf(T[10], rn.z, fmaf(T[6], rn.y, T[2] * rn.x)));
    const float nxx = h.a.w, nxy = h.b.x, nxz = h.b.y, nyy = h.b.z, nyz = h.b.w, nzz = h.c.x;
    // S = C_v + C(u_p) = 2 I - (1 - eps)(N + u_p u_p^T), symmetric: xx xy xz yy yz zz
    const float sxx = 2.f - g * (nxx + up.x * up.x), syy = 2.f - g * (nyy + up.y * up.y), szz = 2.f - g * (nzz + up.z * up.z);
    const float sxy = -g * (nxy + up.x * up.y), sxz = -g * (nxz + up.x * up.z), syz = -g * (nyz + up.y * up.z);
    gicp_pair_sums<false>(acc, sxx, sxy, sxz, syy, syz, szz, p, make_float3(p.x - h.a.x, p.y - h.a.y, p.z - h.a.z), 1.0);
}

__global__ __launch_bounds__(256) void voxel_pairs_kernel(const float4* __restrict__ reading, const float4* __restrict__ read_normals, int n,
                                                          IcpState* __restrict__ st, const uint4* __restrict__ tab, unsigned mask, float size, float eps,
                                                          unsigned* __restrict__ hists)
{
    asm volatile("" ::"s"(reading), "s"(read_normals), "s"(n), "s"(st), "s"(tab), "s"(mask), "s"(size), "s"(eps), "s"(hists));
    unsigned hw = hdr_load(st);
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    // the first two points of every lane and their normals are requested with the header: one trip, the probe is the second.  A lane past
    // the reading loads nothing (an empty reading, or one without a normals array, never has an address formed for it)
    constexpr int PF = 2;
    float4 pr[PF]; float3 pn[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int64_t e = e0 + u * stride;
        const bool in = e < n;
        pr[u] = in ? ld_stream(reading + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        pn[u] = (in && read_normals) ? *reinterpret_cast<const float3*>(read_normals + e) : make_float3(0.f, 0.f, 0.f);
    }
    asm volatile("" : "+v"(hw));
    const HdrView hv{hw};
    const int done = hv.i(ICPMI_HDR_W(done));
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = hv.f(ICPMI_HDR_W(T_iter) + i);
    if (done) return;
    const float g = 1.f - eps;
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    double cnt = 0.0;
    auto pair = [&](float4 r, float3 rn) { voxel_pair(T, r, rn, tab, mask, size, g, acc, cnt); };
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (e0 + u * stride < n) pair(pr[u], pn[u]);
    for (int64_t e = e0 + PF * stride; e < n; e += stride)
        pair(reading[e], read_normals ? *reinterpret_cast<const float3*>(read_normals + e) : make_float3(0.f, 0.f, 0.f));

    pair_sums_fold<256, 27, false>(acc, cnt, cnt, nullptr, hists); // (weight 1 per pair: sum w = the pair count)
}

// The pair sums of a handle with a schedule of two or more levels: voxel_pairs_kernel's body, but for where table, mask
// and size come from.  `sched` is the handle's block of level descriptors (common.h: ICPMI_VS_DESC; 16 dwords, lane l takes dword l & 15),
// requested with the header and the prefetched points in the one first trip; the current level is the header's vox_level, and the
// descriptor's four words are readlanes at 4 * level.  (The level is masked to 0..3 and the host fills all four slots with real tables: no
// value of the word makes the kernel probe an address that is not a table.)  voxel_pairs_kernel keeps serving one-size handles.
__global__ __launch_bounds__(256) void voxel_pairs_sched_kernel(const float4* __restrict__ reading, const float4* __restrict__ read_normals, int n,
                                                                IcpState* __restrict__ st, const unsigned* __restrict__ sched, float eps,
                                                                unsigned* __restrict__ hists)
{
    asm volatile("" ::"s"(reading), "s"(read_normals), "s"(n), "s"(st), "s"(sched), "s"(eps), "s"(hists));
    unsigned hw = hdr_load(st);
    unsigned dw = sched[ICPMI_VS_DESC + (threadIdx.x & 15)];
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    constexpr int PF = 2;
    float4 pr[PF]; float3 pn[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int64_t e = e0 + u * stride;
        const bool in = e < n;
        pr[u] = in ? ld_stream(reading + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        pn[u] = (in && read_normals) ? *reinterpret_cast<const float3*>(read_normals + e) : make_float3(0.f, 0.f, 0.f);
    }
    asm volatile("" : "+v"(hw), "+v"(dw));
    const HdrView hv{hw}, dv{dw};
    const int done = hv.i(ICPMI_HDR_W(done));
    const int lvl = hv.i(ICPMI_HDR_W(vox_level)) & (ICPMI_MAX_VOXEL_LEVELS - 1);
    const uint4* __restrict__ tab = reinterpret_cast<const uint4*>((uintptr_t)dv.u64(4 * lvl));
    const unsigned mask = dv.u(4 * lvl + 2);
    const float size = dv.f(4 * lvl + 3);
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = hv.f(ICPMI_HDR_W(T_iter) + i);
    if (done) return;
    const float g = 1.f - eps;
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    double cnt = 0.0;
    auto pair = [&](float4 r, float3 rn) { voxel_pair(T, r, rn, tab, mask, size, g, acc, cnt); };
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (e0 + u * stride < n) pair(pr[u], pn[u]);
    for (int64_t e = e0 + PF * stride; e < n; e += stride)
        pair(reading[e], read_normals ? *reinterpret_cast<const float3*>(read_normals + e) : make_float3(0.f, 0.f, 0.f));

    pair_sums_fold<256, 27, false>(acc, cnt, cnt, nullptr, hists);
}

// The pair sums of a batch of readings (icpmi_voxel_register_batch_dev, icpmi_voxel_register_multistart*), grid =
// (workgroups of the largest member, members).  blockIdx.y = the member: its slice of the centred readings and of the padded normals
// (ba.qstride), its state, its accumulators.  As in accumulate_kernel a member uses the workgroups -- and the stride -- it has alone
// (acc_blocks of its own n; the grid's other workgroups return at once), so every thread adds the pairs it adds in a single
// registration in the same order, and pair_sums_fold joins fixed-point integers: the member's sums are the bits it has alone.
// The level is the member's own header word; table, mask and size come from `desc`, the 16 descriptor dwords of the handle's batch
// block (a one-size handle uploads one level, repeated in the other slots: one body serves both).  The prologue is
// voxel_pairs_sched_kernel's: header dword, descriptor dword and the first two points and normals of every lane in one trip.  Every
// member has points and normals (api.hip sends a batch with an empty member through the one-by-one route); no lane past a member's
// reading forms an address.
__device__ __forceinline__ int vox_acc_blocks(int n, int cap)
{
    const int nb = (n + 255) / 256; // (loop.hip: acc_blocks_dev with 256 threads)
    return nb < 1 ? 1 : (nb > cap ? cap : nb);
}

// (waves_per_eu: without the hint the allocator takes 98 VGPRs -- two over the 96 of voxel_pairs_sched_kernel and one wave per SIMD fewer;
// with it 96 and no scratch: profiles/voxel_batch_isa_diff.txt)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void voxel_pairs_batch_kernel(const float4* __restrict__ reading, const float4* __restrict__ read_normals, BatchArgs ba,
                                                                int acc_cap, IcpState* __restrict__ st, const unsigned* __restrict__ desc, float eps,
                                                                unsigned* __restrict__ hists)
{
    asm volatile("" ::"s"(ba.n[blockIdx.y]), "s"(ba.qstride), "s"(acc_cap), "s"(reading), "s"(read_normals), "s"(st), "s"(desc), "s"(eps), "s"(hists));
    const int n = ba.n[blockIdx.y];
    const int nbe = vox_acc_blocks(n, acc_cap);
    if ((int)blockIdx.x >= nbe) return;
    {
        const size_t qo = (size_t)blockIdx.y * (size_t)ba.qstride;
        reading += qo; read_normals += qo;
        hists += (size_t)blockIdx.y * ICPMI_SELHIST_WORDS;
        st += blockIdx.y;
    }
    unsigned hw = hdr_load(st);
    unsigned dw = desc[ICPMI_VS_DESC + (threadIdx.x & 15)];
    const int64_t stride = (int64_t)nbe * 256;
    const int64_t e0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    constexpr int PF = 2;
    float4 pr[PF]; float3 pn[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
        const int64_t e = e0 + u * stride;
        const bool in = e < n;
        pr[u] = in ? ld_stream(reading + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        pn[u] = in ? *reinterpret_cast<const float3*>(read_normals + e) : make_float3(0.f, 0.f, 0.f);
    }
    asm volatile("" : "+v"(hw), "+v"(dw));
    const HdrView hv{hw}, dv{dw};
    const int done = hv.i(ICPMI_HDR_W(done));
    const int lvl = hv.i(ICPMI_HDR_W(vox_level)) & (ICPMI_MAX_VOXEL_LEVELS - 1);
    const uint4* __restrict__ tab = reinterpret_cast<const uint4*>((uintptr_t)dv.u64(4 * lvl));
    const unsigned mask = dv.u(4 * lvl + 2);
    const float size = dv.f(4 * lvl + 3);
    float T[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) T[i] = hv.f(ICPMI_HDR_W(T_iter) + i);
    if (done) return;
    const float g = 1.f - eps;
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    double cnt = 0.0;
#pragma unroll
    for (int u = 0; u < PF; ++u)
        if (e0 + u * stride < n) voxel_pair(T, pr[u], pn[u], tab, mask, size, g, acc, cnt);
    for (int64_t e = e0 + PF * stride; e < n; e += stride)
        voxel_pair(T, reading[e], *reinterpret_cast<const float3*>(read_normals + e), tab, mask, size, g, acc, cnt);

    pair_sums_fold<256, 27, false>(acc, cnt, cnt, nullptr, hists);
}

// ---- many poses scored by table lookup (icpmi_voxel_score_poses) ------------------
// A slice is VS_SLICE consecutive reading points (thread t of the workgroup holds the points t, t + 256, ... of its slice): the partition
// of a reading depends on n alone.  A workgroup walks VS_TILE poses over the points it keeps in registers.
constexpr int VS_PPT = 4;                 // points a thread keeps (scripts/voxel_score_bench.py, profiles/voxel_score_sweep.json: 2 / 4 / 8 tried)
constexpr int VS_SLICE = 256 * VS_PPT;
constexpr int VS_TILE = 8;                // poses a workgroup walks (8 / 16 / 32 / 64 tried)
struct VsPartial { double lik, sum; int pairs; float mx; }; // of one (pose, slice); mx = -inf without a pair

__device__ __forceinline__ unsigned lane_xor_bit_u32(unsigned v, int m)
{
    switch (m) {
    case 1: return lane_xor<1>(v);
    case 2: return lane_xor<2>(v);
    case 4: return lane_xor<4>(v);
    case 8: return lane_xor<8>(v);
    case 16: return lane_xor<16>(v);
    default: return lane_xor<32>(v);
    }
}

// One pair's r = d^T M d: voxel_pairs_kernel's arithmetic up to S, then M = adj(S) / det(S) as gicp_pair_sums forms it (a copy: that
// function's sums are not wanted here, and its kernels stay as they are), M d row by row, and the dot product with d -- every product and
// sum in float, left to right, no contraction (include/icpmi.h writes the order out).  false: no pair.
__device__ __forceinline__ bool vs_pair(const float* __restrict__ T, float4 x, float3 rn, const uint4* __restrict__ tab, unsigned mask, float size, float g,
                                        float* r_out)
{
    const float3 p = xf_point(T, x.x, x.y, x.z, x.w);
    unsigned long long key = 0;
    VoxHit h;
    if (!vox_key(p.x, p.y, p.z, size, &key) || !vox_probe(tab, mask, key, &h)) return false;
    const float3 up = unit_or_zero(fmaf(T[8], rn.z, fmaf(T[4], rn.y, T[0] * rn.x)), fmaf(T[9], rn.z, fmaf(T[5], rn.y, T[1] * rn.x)),
                                   fmaf(T[10], rn.z, fmaf(T[6], rn.y, T[2] * rn.x)));
    const float nxx = h.a.w, nxy = h.b.x, nxz = h.b.y, nyy = h.b.z, nyz = h.b.w, nzz = h.c.x;
    const float sxx = 2.f - g * (nxx + up.x * up.x), syy = 2.f - g * (nyy + up.y * up.y), szz = 2.f - g * (nzz + up.z * up.z);
    const float sxy = -g * (nxy + up.x * up.y), sxz = -g * (nxz + up.x * up.z), syz = -g * (nyz + up.y * up.z);
    const float c00 = syy * szz - syz * syz, c01 = sxz * syz - sxy * szz, c02 = sxy * syz - sxz * syy;
    const float c11 = sxx * szz - sxz * sxz, c12 = sxy * sxz - sxx * syz, c22 = sxx * syy - sxy * sxy;
    const float idet = 1.f / (sxx * c00 + sxy * c01 + sxz * c02);
    const float m00 = c00 * idet, m01 = c01 * idet, m02 = c02 * idet, m11 = c11 * idet, m12 = c12 * idet, m22 = c22 * idet;
    const float dx = p.x - h.a.x, dy = p.y - h.a.y, dz = p.z - h.a.z;
    const float mdx = m00 * dx + m01 * dy + m02 * dz, mdy = m01 * dx + m11 * dy + m12 * dz, mdz = m02 * dx + m12 * dy + m22 * dz;
    *r_out = dx * mdx + dy * mdy + dz * mdz;
    return true;
}

// grid = (slices, pose tiles).  poses: 16 floats each, centred frame, uniform over the workgroup (scalar loads).  One VsPartial per
// (pose, slice) at part[pose * slices + slice].  Per pose: every thread adds its points in ascending order, the wave folds in the fixed
// butterfly (lane_xor_bit, m = 1 .. 32), thread 0 adds the four waves in ascending order.  The LDS cells alternate with the pose's parity:
// one barrier per pose.  No lane past the reading forms an address of it.
__global__ __launch_bounds__(256) void voxel_score_kernel(const float4* __restrict__ reading, const float4* __restrict__ normals, int n,
                                                          const float* __restrict__ poses, int n_poses, const uint4* __restrict__ tab, unsigned mask,
                                                          float size, float eps, float hb, VsPartial* __restrict__ part)
{
    __shared__ double sh_d[2][4][2];
    __shared__ int sh_p[2][4];
    __shared__ float sh_m[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * VS_SLICE + threadIdx.x;
    float4 pt[VS_PPT]; float3 nr[VS_PPT];
#pragma unroll
    for (int u = 0; u < VS_PPT; ++u) {
        const int64_t e = e0 + u * 256;
        const bool in = e < n;
        pt[u] = in ? reading[e] : make_float4(0.f, 0.f, 0.f, 0.f);
        nr[u] = in ? *reinterpret_cast<const float3*>(normals + e) : make_float3(0.f, 0.f, 0.f);
    }
    const float g = 1.f - eps;
    const int p0 = (int)blockIdx.y * VS_TILE;
    const int p1 = p0 + VS_TILE < n_poses ? p0 + VS_TILE : n_poses;
    for (int p = p0; p < p1; ++p) {
        const float* __restrict__ T = poses + 16 * (size_t)p;
        double lik = 0.0, sum = 0.0;
        int pairs = 0;
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < VS_PPT; ++u) {
            float r;
            if (e0 + u * 256 < n && vs_pair(T, pt[u], nr[u], tab, mask, size, g, &r)) {
                lik += (double)expf(-(hb * r));
                sum += (double)r;
                ++pairs;
                mx = fmaxf(mx, r);
            }
        }
#pragma unroll
        for (int mk = 1; mk < 64; mk <<= 1) { // (the wave is whole again behind the loop above)
            lik += lane_xor_bit(lik, mk);
            sum += lane_xor_bit(sum, mk);
            pairs += (int)lane_xor_bit_u32((unsigned)pairs, mk);
            mx = fmaxf(mx, __uint_as_float(lane_xor_bit_u32(__float_as_uint(mx), mk)));
        }
        const int b = p & 1;
        if (lane == 0) { sh_d[b][wv][0] = lik; sh_d[b][wv][1] = sum; sh_p[b][wv] = pairs; sh_m[b][wv] = mx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            VsPartial o;
            o.lik = ((sh_d[b][0][0] + sh_d[b][1][0]) + sh_d[b][2][0]) + sh_d[b][3][0];
            o.sum = ((sh_d[b][0][1] + sh_d[b][1][1]) + sh_d[b][2][1]) + sh_d[b][3][1];
            o.pairs = sh_p[b][0] + sh_p[b][1] + sh_p[b][2] + sh_p[b][3];
            o.mx = fmaxf(fmaxf(sh_m[b][0], sh_m[b][1]), fmaxf(sh_m[b][2], sh_m[b][3]));
            part[(size_t)p * gridDim.x + blockIdx.x] = o;
        }
    }
}

// per pose: the slices' partials in ascending slice order, in double; then the result as the caller reads it
__global__ __launch_bounds__(256) void voxel_score_finish_kernel(const VsPartial* __restrict__ part, int n_poses, int slices, int n, int level,
                                                                 icpmi_voxel_score* __restrict__ out)
{
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= n_poses) return;
    double lik = 0.0, sum = 0.0;
    long long pairs = 0;
    float mx = -INFINITY;
    for (int s = 0; s < slices; ++s) {
        const VsPartial v = part[(size_t)p * slices + s];
        lik += v.lik; sum += v.sum; pairs += v.pairs; mx = fmaxf(mx, v.mx);
    }
    icpmi_voxel_score o;
    o.likelihood = lik; o.sum_maha = sum; o.pairs = pairs;
    o.max_maha = pairs > 0 ? mx : 0.f;
    o.pairs_ratio = (float)((double)pairs / (double)n);
    o.level = level;
    o.reserved[0] = o.reserved[1] = o.reserved[2] = 0;
    out[p] = o;
}

// the HIP events of a timed diagnostic: created together, destroyed on every way out of the call
template <int N>
struct EventSet {
    hipEvent_t ev[N] = {};
    EventSet() = default;
    EventSet(const EventSet&) = delete;
    EventSet& operator=(const EventSet&) = delete;
    ~EventSet() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    hipError_t create() { for (hipEvent_t& e : ev) { const hipError_t s = hipEventCreate(&e); if (s != hipSuccess) { e = nullptr; return s; } } return hipSuccess; }
};

} // namespace

static bool voxel_level_current(const icpmi_ctx* c, int l)
{
    const VoxLevel& v = c->vox[l];
    return v.ready && v.nv > 0 && v.map_version == c->map_version && v.epoch == c->map_epoch && v.built_size == c->vox_sizes[l];
}

bool voxel_table_current(const icpmi_ctx* c)
{
    for (int l = 0; l < c->vox_levels; ++l) if (!voxel_level_current(c, l)) return false;
    return c->vox_levels > 0;
}

// Builds level l's table of the resident map for c->vox_sizes[l] unless the handle holds it already (lazily: the first call that needs it
// after the map or the size changed).  Stream-ordered but for one read-back (voxel count and range flag).  times_ms (may be null): sort,
// reduce, fill as HIP events measure them (scripts/voxel_bench.py); asking for them forces a rebuild.
static icpmi_status voxel_ensure_level(icpmi_ctx* c, int l, float* times_ms)
{
    VoxLevel& lv = c->vox[l];
    const float size = c->vox_sizes[l];
    if (!times_ms && voxel_level_current(c, l)) return ICPMI_OK;
    lv.ready = false;
    const int64_t m = c->m;
    const int blocks = (int)((m + 255) / 256);
    unsigned long long* d_keys = scratch_get<unsigned long long>(c, 0, (size_t)2 * m + 2);
    unsigned* d_vals = scratch_get<unsigned>(c, 1, (size_t)2 * m + 2);
    unsigned* d_tab = scratch_get<unsigned>(c, 2, radix_sort_tab_words(m, 63));
    const int64_t fs = m + 2; // the scan writes out[m] (its total) behind its output
    unsigned* d_flag = scratch_get<unsigned>(c, 4, (size_t)2 * fs + 4); // head | pos | range flag
    unsigned* d_vstart = scratch_get<unsigned>(c, 5, (size_t)m + 2);
    if (!d_keys || !d_vals || !d_tab || !d_flag || !d_vstart) return ICPMI_ERR_HIP;
    unsigned* d_head = d_flag; unsigned* d_pos = d_flag + fs; unsigned* d_bad = d_flag + 2 * fs;
    EventSet<4> evs; // (destroyed on every way out)
    hipEvent_t* ev = evs.ev;
    if (times_ms) HIP_TRY(c, evs.create());

    HIP_TRY(c, hipMemsetAsync(d_bad, 0, sizeof(unsigned), c->stream));
    if (ev[0]) (void)hipEventRecord(ev[0], c->stream);
    hipLaunchKernelGGL(vox_key_kernel, dim3(blocks), dim3(256), 0, c->stream, (const float4*)c->d_map_sorted, m, size, d_keys, d_vals, d_bad);
    HIP_TRY(c, hipGetLastError());
    int half = 0;
    { const icpmi_status s = radix_sort_pairs(c, d_keys, d_vals, m, 63, d_tab, &half); if (s != ICPMI_OK) return s; }
    const unsigned long long* skeys = d_keys + (half ? m : 0);
    const unsigned* svals = d_vals + (half ? m : 0);
    hipLaunchKernelGGL(vox_head_kernel, dim3(blocks), dim3(256), 0, c->stream, skeys, m, d_head);
    HIP_TRY(c, hipGetLastError());
    if (ev[1]) (void)hipEventRecord(ev[1], c->stream);
    int64_t nv = 0;
    { const icpmi_status s = device_scan_flags_count(c, d_head, d_pos, (int)m, &nv); if (s != ICPMI_OK) return s; }
    unsigned bad = 0;
    if (read_back(c, &bad, d_bad, sizeof bad) != ICPMI_OK) return ICPMI_ERR_HIP;
    if (bad) {
        c->last_error = "voxel matcher: a map point has a non-finite coordinate or lies 2^20 or more voxels from the map's centroid on one axis";
        return ICPMI_ERR_INVALID_ARG;
    }
    if (nv <= 0 || nv > m) { c->last_error = "voxel matcher: bad voxel count"; return ICPMI_ERR_HIP; }
    unsigned cap = 2;
    while ((uint64_t)cap < 2 * (uint64_t)nv) cap <<= 1;
    if (lv.keys.ensure(c, (size_t)nv) != ICPMI_OK || lv.rec.ensure(c, (size_t)3 * nv) != ICPMI_OK ||
        lv.tab.ensure(c, (size_t)4 * cap) != ICPMI_OK) return ICPMI_ERR_HIP;
    hipLaunchKernelGGL(vox_start_kernel, dim3(blocks), dim3(256), 0, c->stream, (const unsigned*)d_head, (const unsigned*)d_pos, m, d_vstart);
    hipLaunchKernelGGL(vox_reduce_kernel, dim3((int)((nv + 3) / 4)), dim3(256), 0, c->stream, skeys, svals, (const unsigned*)d_vstart, nv,
                       (const float4*)c->d_map_sorted, (const float4*)c->d_normals_sorted, lv.keys.get(), lv.rec.get());
    HIP_TRY(c, hipGetLastError());
    if (ev[2]) (void)hipEventRecord(ev[2], c->stream);
    HIP_TRY(c, hipMemsetAsync(lv.tab.get(), 0xff, (size_t)cap * 64, c->stream));
    hipLaunchKernelGGL(vox_fill_kernel, dim3((int)((nv + 255) / 256)), dim3(256), 0, c->stream, (const unsigned long long*)lv.keys.get(),
                       (const float4*)lv.rec.get(), nv, lv.tab.get(), cap - 1);
    HIP_TRY(c, hipGetLastError());
    if (ev[3]) (void)hipEventRecord(ev[3], c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (times_ms) {
        for (int i = 0; i < 3; ++i) { times_ms[i] = 0.f; (void)hipEventElapsedTime(&times_ms[i], ev[i], ev[i + 1]); }
    }
    lv.nv = nv; lv.mask = cap - 1;
    lv.map_version = c->map_version; lv.epoch = c->map_epoch; lv.built_size = size;
    ++lv.gen;
    lv.ready = true;
    return ICPMI_OK;
}

// Every level of the handle's schedule, by the one build path, coarsest first; then, with two or more levels, the level descriptors on the
// device (uploaded again whenever a table or a size is not the one they describe).  times_ms: the finest level's build, forced.
icpmi_status voxel_ensure_table(icpmi_ctx* c, float* times_ms)
{
    if (c->vox_levels <= 0 || !(c->voxel_size > 0.f)) { c->last_error = "voxel matcher: no voxel size set (icpmi_set_voxel_matcher)"; return ICPMI_ERR_INVALID_ARG; }
    if (c->m <= 0) { c->last_error = "voxel matcher: no map"; return ICPMI_ERR_INVALID_ARG; }
    if (!c->has_normals || !c->d_normals_sorted.get()) {
        c->last_error = "InvalidField: VoxelMatcher needs the descriptor 'normals' on the map"; return ICPMI_ERR_MISSING_NORMALS;
    }
    const int L = c->vox_levels;
    for (int l = 0; l < L; ++l) {
        const icpmi_status s = voxel_ensure_level(c, l, l == L - 1 ? times_ms : nullptr);
        if (s != ICPMI_OK) return s;
    }
    if (L < 2) return ICPMI_OK;
    unsigned desc[4 * ICPMI_MAX_VOXEL_LEVELS];
    for (int l = 0; l < ICPMI_MAX_VOXEL_LEVELS; ++l) { // (the slots behind the last level repeat it: whatever the level word holds, the kernel probes a real table)
        const int src = l < L ? l : L - 1;
        const unsigned long long a = (unsigned long long)(uintptr_t)c->vox[src].tab.get();
        desc[4 * l + 0] = (unsigned)a; desc[4 * l + 1] = (unsigned)(a >> 32); desc[4 * l + 2] = c->vox[src].mask;
        memcpy(desc + 4 * l + 3, c->vox_sizes + src, sizeof(float));
    }
    const uint64_t sig = voxel_sched_sig(c, 0);
    if (c->d_vox_sched.get() && c->vox_sched_sig == sig) return ICPMI_OK;
    if (c->d_vox_sched.ensure(c, ICPMI_VS_WORDS) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemsetAsync(c->d_vox_sched.get(), 0, ICPMI_VS_WORDS * sizeof(unsigned), c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_vox_sched.get() + ICPMI_VS_DESC, desc, sizeof desc, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (desc is on this frame)
    c->vox_sched_sig = voxel_sched_sig(c, 0);
    return ICPMI_OK;
}

// what a captured loop, and the uploaded descriptors, are valid for on the voxel path: the level count and every level's size, table
// generation and table address (h: the hash so far)
uint64_t voxel_sched_sig(const icpmi_ctx* c, uint64_t h)
{
    h = fnv(&c->vox_levels, sizeof c->vox_levels, h ? h : 1469598103934665603ull);
    for (int l = 0; l < c->vox_levels; ++l) {
        const void* tab = c->vox[l].tab.get();
        h = fnv(&c->vox_sizes[l], sizeof(float), h);
        h = fnv(&c->vox[l].gen, sizeof c->vox[l].gen, h);
        h = fnv(&tab, sizeof tab, h);
    }
    return h;
}

// the iteration's pair sums on the handle's stream (no allocation, no wait: loop.hip captures it); the table is current (voxel_ensure_table)
void voxel_enqueue_pairs(icpmi_ctx* c, int64_t n, int nb, float eps)
{
    if (c->vox_levels >= 2) { // (a schedule: the level is read on the device)
        hipLaunchKernelGGL(voxel_pairs_sched_kernel, dim3(nb), dim3(256), 0, c->stream, (const float4*)c->d_reading, (const float4*)c->d_read_normals, (int)n,
                           c->d_state.get(), (const unsigned*)c->d_vox_sched.get(), eps, c->d_selhist.get());
        return;
    }
    hipLaunchKernelGGL(voxel_pairs_kernel, dim3(nb), dim3(256), 0, c->stream, (const float4*)c->d_reading, (const float4*)c->d_read_normals, (int)n,
                       c->d_state.get(), (const uint4*)c->vox[0].tab.get(), c->vox[0].mask, c->voxel_size, eps, c->d_selhist.get());
}

// The device block of a batch (common.h: icpmi_ctx::d_vox_batch): ICPMI_VS_WORDS dwords whose descriptor part every member reads -- for a
// one-size handle too: its one level in all four slots -- and behind them one block of ICPMI_VS_WORDS per member, whose report part
// (ICPMI_VS_BASE ..) is that member's.  The tables are current (voxel_ensure_table); uploaded again when they, or the sizes, change.
// Allocates and waits: before anything of the batch is enqueued.
icpmi_status voxel_ensure_batch_block(icpmi_ctx* c)
{
    const int L = c->vox_levels;
    unsigned desc[4 * ICPMI_MAX_VOXEL_LEVELS];
    for (int l = 0; l < ICPMI_MAX_VOXEL_LEVELS; ++l) {
        const int src = l < L ? l : L - 1;
        const unsigned long long a = (unsigned long long)(uintptr_t)c->vox[src].tab.get();
        desc[4 * l + 0] = (unsigned)a; desc[4 * l + 1] = (unsigned)(a >> 32); desc[4 * l + 2] = c->vox[src].mask;
        memcpy(desc + 4 * l + 3, c->vox_sizes + src, sizeof(float));
    }
    const uint64_t sig = voxel_sched_sig(c, 0);
    if (c->d_vox_batch.get() && c->vox_batch_sig == sig) return ICPMI_OK;
    constexpr size_t words = (size_t)ICPMI_VS_WORDS * (1 + ICPMI_MAX_BATCH);
    if (c->d_vox_batch.ensure(c, words) != ICPMI_OK) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemsetAsync(c->d_vox_batch.get(), 0, words * sizeof(unsigned), c->stream));
    HIP_TRY(c, hipMemcpyAsync(c->d_vox_batch.get() + ICPMI_VS_DESC, desc, sizeof desc, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (desc is on this frame)
    c->vox_batch_sig = sig;
    return ICPMI_OK;
}

// the pair sums of a batch's iteration on the handle's stream (no allocation, no wait); nmax = the largest member, cap = loop.hip's acc_cap
void voxel_enqueue_pairs_batch(icpmi_ctx* c, const BatchArgs& ba, int nb, int cap, float eps)
{
    hipLaunchKernelGGL(voxel_pairs_batch_kernel, dim3(nb, ba.nscan), dim3(256), 0, c->stream, (const float4*)c->d_reading, (const float4*)c->d_read_normals, ba,
                       cap, c->d_state.get(), (const unsigned*)c->d_vox_batch.get(), eps, c->d_selhist.get());
}

// level: of the schedule, 0 the coarsest; -1 the finest
static icpmi_status voxel_level_arg(icpmi_ctx* c, const char* who, int* level)
{
    if (*level == -1) *level = c->vox_levels - 1;
    if (*level < 0 || *level >= c->vox_levels) { c->last_error = std::string(who) + ": no such level in the voxel schedule"; return ICPMI_ERR_INVALID_ARG; }
    return ICPMI_OK;
}

icpmi_status voxel_get_map(icpmi_ctx* c, int level, int64_t cap, int32_t* ijk3, float* mean3, float* moments6, int32_t* count, int64_t* n_voxels)
{
    { const icpmi_status s = voxel_ensure_table(c, nullptr); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = voxel_level_arg(c, "get_voxel_map", &level); if (s != ICPMI_OK) return s; }
    const VoxLevel& lv = c->vox[level];
    const int64_t nv = lv.nv;
    if (n_voxels) *n_voxels = nv;
    if (cap < nv) { c->last_error = "get_voxel_map: capacity below the voxel count (*n_voxels has it)"; return ICPMI_ERR_INVALID_ARG; }
    std::vector<unsigned long long> keys((size_t)nv);
    std::vector<float> rec((size_t)12 * nv);
    HIP_TRY(c, hipMemcpyAsync(keys.data(), lv.keys.get(), (size_t)nv * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(rec.data(), lv.rec.get(), (size_t)nv * 12 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t v = 0; v < nv; ++v) {
        const float* r = rec.data() + 12 * v;
        if (ijk3) {
            ijk3[3 * v + 0] = (int)((keys[v] >> 42) & 0x1fffff) - VOX_BIAS;
            ijk3[3 * v + 1] = (int)((keys[v] >> 21) & 0x1fffff) - VOX_BIAS;
            ijk3[3 * v + 2] = (int)(keys[v] & 0x1fffff) - VOX_BIAS;
        }
        if (mean3) for (int j = 0; j < 3; ++j) mean3[3 * v + j] = r[j];
        if (moments6) for (int j = 0; j < 6; ++j) moments6[6 * v + j] = r[3 + j];
        if (count) { unsigned cw; memcpy(&cw, r + 9, sizeof cw); count[v] = (int32_t)cw; }
    }
    return ICPMI_OK;
}

icpmi_status voxel_lookup(icpmi_ctx* c, int level, const float* q4_centred, int64_t n, int32_t* voxel)
{
    { const icpmi_status s = voxel_ensure_table(c, nullptr); if (s != ICPMI_OK) return s; }
    { const icpmi_status s = voxel_level_arg(c, "voxel_lookup", &level); if (s != ICPMI_OK) return s; }
    const VoxLevel& lv = c->vox[level];
    if (n == 0) return ICPMI_OK;
    DevBuf<float4> d_q; DevBuf<int> d_out;
    HIP_TRY(c, d_q.alloc((size_t)n));
    HIP_TRY(c, d_out.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(d_q.get(), q4_centred, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(vox_lookup_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, (const float4*)d_q.get(), n, c->vox_sizes[level],
                       (const uint4*)lv.tab.get(), lv.mask, d_out.get());
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(voxel, d_out.get(), (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ICPMI_OK;
}

void voxel_score_shape(int32_t* slice, int32_t* tile) { *slice = VS_SLICE; *tile = VS_TILE; }

// icpmi_voxel_score_poses*: centre and pad the reading once, one scoring launch over (slices, pose tiles), the finish, one read-back.
// Everything lives in the operator scratch (slots 10 .. 14): the handle's reading, loop state and captured loop stay what they were.
icpmi_status voxel_score_poses(icpmi_ctx* c, const float4* d_scan, int64_t n, const float* d_n3, const float* Tc, int n_poses, int level, float hb,
                               icpmi_voxel_score* out)
{
    const VoxLevel& lv = c->vox[level];
    const int slices = (int)((n + VS_SLICE - 1) / VS_SLICE);
    const int tiles = (n_poses + VS_TILE - 1) / VS_TILE;
    float4* d_pts = scratch_get<float4>(c, 10, (size_t)n);
    float4* d_nrm = scratch_get<float4>(c, 11, (size_t)n);
    float* d_T = scratch_get<float>(c, 12, (size_t)16 * n_poses);
    VsPartial* d_part = scratch_get<VsPartial>(c, 13, (size_t)n_poses * slices);
    icpmi_voxel_score* d_out = scratch_get<icpmi_voxel_score>(c, 14, (size_t)n_poses);
    if (!d_pts || !d_nrm || !d_T || !d_part || !d_out) return ICPMI_ERR_HIP;
    { const icpmi_status s = loop_centre_pad(c, d_scan, n, d_n3, d_pts, d_nrm); if (s != ICPMI_OK) return s; }
    HIP_TRY(c, hipMemcpyAsync(d_T, Tc, (size_t)16 * n_poses * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(voxel_score_kernel, dim3(slices, tiles), dim3(256), 0, c->stream, (const float4*)d_pts, (const float4*)d_nrm, (int)n,
                       (const float*)d_T, n_poses, (const uint4*)lv.tab.get(), lv.mask, c->vox_sizes[level], c->plane_eps, hb, d_part);
    hipLaunchKernelGGL(voxel_score_finish_kernel, dim3((n_poses + 255) / 256), dim3(256), 0, c->stream, (const VsPartial*)d_part, n_poses, slices, (int)n,
                       level, d_out);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out, (size_t)n_poses * sizeof(icpmi_voxel_score), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // (Tc is the caller's until here)
    return ICPMI_OK;
}

// diagnostics (scripts/voxel_bench.py): n centred-frame queries looked up `reps` times through the table and `reps` times by binary search
// over the sorted keys; ms[0] / ms[1] = the mean milliseconds of one launch of either, *mismatch = queries the two answer differently
icpmi_status voxel_lookup_times(icpmi_ctx* c, const float* q4_centred, int64_t n, int reps, float ms[2], int64_t* mismatch)
{
    { const icpmi_status s = voxel_ensure_table(c, nullptr); if (s != ICPMI_OK) return s; }
    const VoxLevel& lv = c->vox[c->vox_levels - 1]; // (the finest level)
    DevBuf<float4> d_q; DevBuf<int> d_a, d_b;
    HIP_TRY(c, d_q.alloc((size_t)n));
    HIP_TRY(c, d_a.alloc((size_t)n));
    HIP_TRY(c, d_b.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(d_q.get(), q4_centred, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    EventSet<3> evs; // (destroyed on every way out)
    hipEvent_t* ev = evs.ev;
    HIP_TRY(c, evs.create());
    const dim3 grid((int)((n + 255) / 256));
    for (int pass = 0; pass < 2; ++pass) { // (pass 0 warms both)
        (void)hipEventRecord(ev[0], c->stream);
        for (int r = 0; r < reps; ++r)
            hipLaunchKernelGGL(vox_lookup_kernel, grid, dim3(256), 0, c->stream, (const float4*)d_q.get(), n, c->voxel_size, (const uint4*)lv.tab.get(),
                               lv.mask, d_a.get());
        (void)hipEventRecord(ev[1], c->stream);
        for (int r = 0; r < reps; ++r)
            hipLaunchKernelGGL(vox_lookup_bsearch_kernel, grid, dim3(256), 0, c->stream, (const float4*)d_q.get(), n, c->voxel_size,
                               (const unsigned long long*)lv.keys.get(), lv.nv, d_b.get());
        (void)hipEventRecord(ev[2], c->stream);
    }
    const hipError_t se = hipStreamSynchronize(c->stream);
    ms[0] = ms[1] = 0.f;
    (void)hipEventElapsedTime(&ms[0], ev[0], ev[1]);
    (void)hipEventElapsedTime(&ms[1], ev[1], ev[2]);
    HIP_TRY(c, se);
    HIP_TRY(c, hipGetLastError());
    ms[0] /= (float)reps; ms[1] /= (float)reps;
    std::vector<int> a((size_t)n), b((size_t)n);
    HIP_TRY(c, hipMemcpy(a.data(), d_a.get(), (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(b.data(), d_b.get(), (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) bad += a[(size_t)i] != b[(size_t)i];
    if (mismatch) *mismatch = bad;
    return ICPMI_OK;
}
