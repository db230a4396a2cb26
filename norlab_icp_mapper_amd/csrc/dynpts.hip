// dynpts.hip -- DynamicPointsMapperModule: the probability of being dynamic of every map point a scan's beams pass near.  Self-contained: its
// own angular bucket grid, three kernels, its own scratch slots (10..19) and -- from the map-update chain (ops.hip) -- a side stream.
#include "common.h"

namespace {

// ---- DynamicPointsMapperModule::inPlaceUpdateMap (DynamicPointsMapperModule.cpp:34-172) -------------------
// Beams = input points in the sensor frame as (elevation, azimuth); every in-range map point looks up
// its angularly nearest beam within 2 * beamHalfAngle (the reference builds a 2-D kd-tree per call,
// :75-78; here: a bucket grid of that cell size built by counting sort, 3 x 3 cells per query, ties to
// the smallest beam index) and updates its probability of being dynamic (:97-148).
// asin / atan2 go through double and are rounded once (shared with the oracle: libm and the device
// library then agree bit for bit); everything else is the reference's float arithmetic, with the
// sub-expressions it writes with a double literal (`1.`) evaluated in double.
#ifndef DYN_RINGS
#define DYN_RINGS 2   // buckets per search radius (1: 3 x 3 block of one-radius buckets, the layout until r4)
#endif
struct DynGrid { float cell; int ne, na; float r2; };   // r2 = (2 beamHalfAngle)^2: the search radius, just under DYN_RINGS cells
constexpr int64_t DYN_MAX_CELLS = 1ll << 28;

// The grid of a half angle and its number of buckets: the ONE place either comes from (dynpts_dev sizes its tables with it, dynpts_side_ok
// picks the scan route by it, dynpts_check refuses by it).  More than DYN_MAX_CELLS buckets: g is not usable (the counts of a half angle
// near zero fit no integer; they stay floats until they are known to be small).
int64_t dyn_grid(const icpmi_dynpts_params* prm, DynGrid& g)
{
    const float reach = 2 * prm->beam_half_angle;
    g.r2 = reach * reach;
    // A bucket is a little WIDER than reach / DYN_RINGS.  The bucket of an angle is floorf((angle + c) / cell) in float32: a sum and a
    // quotient that round, by up to 2e-3 buckets for the smallest half angle served.  With buckets of exactly half the reach, a point one
    // ulp below a bucket edge was rounded UP into the bucket above while a beam just under 2 * beamHalfAngle below it stayed where it
    // was: three buckets apart, outside the (2 R + 1)^2 block, and the search missed a beam the reference finds.  1 / 256 of slack per
    // bucket keeps every beam within the reach inside the block whatever the rounding does (R / 256 = 7.8e-3 buckets to spare).
    g.cell = reach / (float)DYN_RINGS * (1.f + 1.f / 256.f);
    const float fe = floorf(3.14159265358979f / g.cell) + 2.f, fa = floorf(6.28318530717959f / g.cell) + 2.f;
    if (!(fe <= (float)DYN_MAX_CELLS && fa <= (float)DYN_MAX_CELLS)) { g.ne = g.na = 0; return INT64_MAX; }
    g.ne = (int)fe; g.na = (int)fa;   // (exact: both are integers below 2^24 wherever the product passes the limit)
    return (int64_t)g.ne * g.na;
}

__device__ __forceinline__ void to_spherical(float x, float y, float z, float& radius, float& elev, float& azim)
{
    radius = sqrtf(x * x + y * y + z * z);
    elev = (float)asin((double)(z / radius));
    azim = (float)atan2((double)y, (double)x);
}

__device__ __forceinline__ int dyn_ecell(const DynGrid& g, float e)
{
    const int v = (int)floorf((e + 1.5707963267949f) / g.cell);
    return v < 0 ? 0 : (v > g.ne - 1 ? g.ne - 1 : v);
}
__device__ __forceinline__ int dyn_acell(const DynGrid& g, float a)
{
    const int v = (int)floorf((a + 3.14159265358979f) / g.cell);
    return v < 0 ? 0 : (v > g.na - 1 ? g.na - 1 : v);
}

// pass 1: beams to the sensor frame + angles + cell counts
__global__ __launch_bounds__(256) void dyn_beams_kernel(const float4* __restrict__ in, int64_t n, Mat16 M, DynGrid g,
                                                        float4* __restrict__ beam_xyzn, float2* __restrict__ beam_ang,
                                                        unsigned* __restrict__ keys, unsigned* __restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const float4 p = in[valid ? i : 0];
    const float3 o = xf_point(M.v, p.x, p.y, p.z, p.w);
    float radius, elev, azim;
    to_spherical(o.x, o.y, o.z, radius, elev, azim);
    const unsigned key = (unsigned)(dyn_ecell(g, elev) * g.na + dyn_acell(g, azim));
    // a lidar scan is ordered along its beams: neighbours in the array fall into the same bucket, and same-address device atomics
    // serialise -- one atomic per run of equal keys in the wave (r5; map_build.hip's counting sorts do the same)
    const WaveRun r = wave_run(key, valid);
    if (r.head) atomicAdd(&count[key], (unsigned)r.len);
    if (!valid) return;
    beam_xyzn[i] = make_float4(o.x, o.y, o.z, radius);
    beam_ang[i] = make_float2(elev, azim);
    keys[i] = key;
}

// pass 2: counting-sort scatter; a bucket entry is ONE 16-byte record {elevation, azimuth, beam index} (r5: the index used to sit in a second
// array -- a dependent load per accepted candidate); the buckets of one elevation row are contiguous, so a row of the 3 x 3 block is one run
__global__ __launch_bounds__(256) void dyn_scatter_kernel(int64_t n, const unsigned* __restrict__ keys, unsigned* __restrict__ cursor /* = starts + 1 */,
                                                          const float2* __restrict__ beam_ang, float4* __restrict__ sorted_rec)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    const unsigned key = keys[valid ? i : 0];
    const float2 a = beam_ang[valid ? i : 0];
    const WaveRun r = wave_run(key, valid);
    unsigned base = 0;
    if (r.head) base = atomicAdd(&cursor[key], (unsigned)r.len);
    base = (unsigned)__shfl((int)base, r.head_lane, 64);
    if (!valid) return;
    sorted_rec[base + (unsigned)r.rank] = make_float4(a.x, a.y, __uint_as_float((unsigned)i), 0.f);
}

#ifndef DYN_INFLIGHT
#define DYN_INFLIGHT 4
#endif
struct DynPrm { float threshold_dynamic, alpha, beta, beam_half_angle, epsilon_a, epsilon_d, sensor_max_range; };

__global__ __launch_bounds__(256) void dyn_update_kernel(const float4* __restrict__ map, const float* __restrict__ normals3, int64_t m,
                                                         Mat16 M, DynGrid g, DynPrm prm,
                                                         const float4* __restrict__ beam_xyzn, const float4* __restrict__ sorted_rec,
                                                         const unsigned* __restrict__ start, float* __restrict__ prob)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float* T = M.v;
    const float eps = 0.0001f;
    const float4 mpt = map[i];
    const float3 mp = xf_point(T, mpt.x, mpt.y, mpt.z, mpt.w);
    const float mapNorm = sqrtf(mp.x * mp.x + mp.y * mp.y + mp.z * mp.z);
    if (!(mapNorm < prm.sensor_max_range)) return; // range cull (:60-69)
    float radius, qe, qa;
    to_spherical(mp.x, mp.y, mp.z, radius, qe, qa);
    const int ce = dyn_ecell(g, qe), ca = dyn_acell(g, qa);
    const float r2 = g.r2;
    float bd = INFINITY;
    int best = -1;
    // The nearest beam within 2 * beamHalfAngle = DYN_RINGS bucket edges: it lies in the (2 R + 1)^2 block of buckets around the point's
    // own.  The buckets (e, a - R .. a + R) of one elevation row are consecutive keys: the bounds of a row's buckets are 2 R + 2 consecutive
    // words, and all of them are requested together before anything depends on them (r4 fetched the two bounds of a bucket when it got
    // there: nine dependent round trips before the ninth bucket's records).  Own bucket first, then ring by ring: where the beams are
    // dense the nearest one is a fraction of a bucket away, and a bucket whose nearest edge is farther than the best so far cannot hold a
    // closer beam (nor an equally close one: the test is strict and leaves a margin for the rounding of the cell assignment).  The winner
    // is the minimum of (angular distance, beam index): independent of the visiting order.
    // r5: buckets of HALF the radius (R = 2, 5 x 5 block).  With one-radius buckets a point paid for every record of its own bucket before
    // the pruning could start -- 150 records where a surface is seen at a grazing angle (the synthetic scenes; a spinning lidar's own
    // returns are uniform in angle); a quarter bucket first, and the ring behind it mostly pruned: search 136 -> see DESIGN 13.2b.
    // (Scanning whole rows without the per-bucket test -- fewer branches -- looked at 3 - 5 x the records and was slower: 253 vs 225 us.)
    constexpr int R = DYN_RINGS, W = 2 * R + 1;
    const float elo = (float)ce * g.cell - 1.5707963267949f, alo = (float)ca * g.cell - 3.14159265358979f;
    float gapE[W], gapA[W];
#pragma unroll
    for (int d = 0; d < W; ++d) {
        // distance from the query to the nearest edge of the bucket d - R cells away (0 for its own)
        gapE[d] = d < R ? (qe - elo) + (float)(R - 1 - d) * g.cell : (d == R ? 0.f : (elo + g.cell - qe) + (float)(d - R - 1) * g.cell);
        gapA[d] = d < R ? (qa - alo) + (float)(R - 1 - d) * g.cell : (d == R ? 0.f : (alo + g.cell - qa) + (float)(d - R - 1) * g.cell);
    }
    unsigned sb[W][W + 1];
#pragma unroll
    for (int de = 0; de < W; ++de) {
        const int e = ce + de - R;
        const bool row = e >= 0 && e < g.ne;
#pragma unroll
        for (int x = 0; x <= W; ++x) {
            int a = ca - R + x;                       // bound x = start of bucket (e, ca - R + x)
            a = a < 0 ? 0 : (a > g.na ? g.na : a);    // (a == na: the start of the next row's first bucket = the end of this row's last)
            sb[de][x] = start[row ? (unsigned)(e * g.na + a) : 0u];
        }
    }
#pragma unroll
    for (int ring = 0; ring <= R; ++ring) {
#pragma unroll
        for (int de = 0; de < W; ++de) {
#pragma unroll
            for (int da = 0; da < W; ++da) {
                const int re = de > R ? de - R : R - de, ra = da > R ? da - R : R - da;
                if ((re > ra ? re : ra) != ring) continue;   // (compile time)
                const int e = ce + de - R, a = ca + da - R;
                if (e < 0 || e >= g.ne || a < 0 || a >= g.na) continue;
                const float ge = fmaxf(gapE[de] - 1e-5f, 0.f), ga = fmaxf(gapA[da] - 1e-5f, 0.f);
                const float dmin = ge * ge + ga * ga;
                if (dmin > r2 || dmin > bd) continue;
                // DYN_INFLIGHT records requested together (r5: one per trip made every record a full memory round trip of the wave's slowest lane)
                const unsigned jend = sb[de][da + 1];
                for (unsigned j = sb[de][da]; j < jend; j += DYN_INFLIGHT) {
                    float4 rec[DYN_INFLIGHT];
#pragma unroll
                    for (int u = 0; u < DYN_INFLIGHT; ++u) rec[u] = sorted_rec[j + u < jend ? j + u : jend - 1];
#pragma unroll
                    for (int u = 0; u < DYN_INFLIGHT; ++u) {
                        const float d0 = qe - rec[u].x, d1 = qa - rec[u].y;
                        const float d = d0 * d0 + d1 * d1;
                        if (d <= r2 && d <= bd) { // ties on the angular distance go to the smallest beam index (the bucket order is arbitrary; a clamped repeat changes nothing)
                            const int b = (int)__float_as_uint(rec[u].z);
                            if (d < bd || b < best) { bd = d; best = b; }
                        }
                    }
                }
            }
        }
    }
    if (best < 0) return; // no beam within 2 * beamHalfAngle

    const float4 ip = beam_xyzn[best];
    const float inputNorm = ip.w;
    const float dx = ip.x - mp.x, dy = ip.y - mp.y, dz = ip.z - mp.z;
    const float delta = sqrtf(dx * dx + dy * dy + dz * dz);
    const float d_max = prm.epsilon_a * inputNorm;
    const float n0 = normals3[3 * i], n1 = normals3[3 * i + 1], n2 = normals3[3 * i + 2];
    const float nx = fmaf(T[8], n2, fmaf(T[4], n1, T[0] * n0));
    const float ny = fmaf(T[9], n2, fmaf(T[5], n1, T[1] * n0));
    const float nz = fmaf(T[10], n2, fmaf(T[6], n1, T[2] * n0));
    const float ndot = (nx * mp.x + ny * mp.y + nz * mp.z) / mapNorm;

    const float w_v = (float)(eps + (1. - eps) * fabs((double)ndot));
    const float w_d1 = (float)(eps + (1. - eps) * (1. - sqrtf(bd) / (2 * prm.beam_half_angle)));
    const float offset = delta - prm.epsilon_d;
    float w_d2 = 1.f;
    if (delta < prm.epsilon_d || mapNorm > inputNorm) w_d2 = eps;
    else if (offset < d_max) w_d2 = eps + (1 - eps) * offset / d_max;
    float w_p2 = eps;
    if (delta < prm.epsilon_d) w_p2 = 1.f;
    else if (offset < d_max) w_p2 = (float)(eps + (1. - eps) * (1. - offset / d_max));

    if ((inputNorm + prm.epsilon_d + d_max) >= mapNorm) {
        const float lastDyn = prob[i];
        const float c1 = 1 - (w_v * w_d1);
        const float c2 = w_v * w_d1;
        float probDynamic, probStatic;
        if (lastDyn < prm.threshold_dynamic) {
            probDynamic = c1 * lastDyn + c2 * w_d2 * ((1 - prm.alpha) * (1 - lastDyn) + prm.beta * lastDyn);
            probStatic = c1 * (1 - lastDyn) + c2 * w_p2 * (prm.alpha * (1 - lastDyn) + (1 - prm.beta) * lastDyn);
        } else { // latched: once dynamic, always dynamic
            probDynamic = 1 - eps;
            probStatic = eps;
        }
        prob[i] = probDynamic / (probDynamic + probStatic);
    }
}

} // namespace

// DynamicPointsMapperModule::inPlaceUpdateMap on DEVICE arrays (T = pose^-1 as a kernel argument); d_prob updated in place.  Its scratch is
// its own (slots 10..19) and `stream` may be the handle's side stream: the module only touches the probabilities of the OLD map points, so
// the map-update chain runs it next to the decimation that follows (ops_map_update_chain).
icpmi_status dynpts_dev(icpmi_ctx* c, const icpmi_dynpts_params* prm, const float T[16], const float4* d_in, int64_t n,
                               const float4* d_map, const float* d_nrm, int64_t m, float* d_prob, hipStream_t stream)
{
    if (n == 0 || m == 0) return ICPMI_OK; // "if (beams.empty()) return"
    DynGrid g;
    const int64_t ncells = dyn_grid(prm, g);
    if (ncells > DYN_MAX_CELLS) return dynpts_check(c, prm); // (the chain has asked already; the stage entry has not)
    DynPrm dp = {prm->threshold_dynamic, prm->alpha, prm->beta, prm->beam_half_angle, prm->epsilon_a, prm->epsilon_d, prm->sensor_max_range};
    float4* d_bx = scratch_get<float4>(c, 10, (size_t)n);
    float2* d_ba = scratch_get<float2>(c, 11, (size_t)n);
    unsigned* d_keys = scratch_get<unsigned>(c, 12, (size_t)n);
    unsigned* d_start = scratch_get<unsigned>(c, 13, (size_t)ncells + 2);
    unsigned* d_cnt = scratch_get<unsigned>(c, 14, (size_t)ncells + 2);
    float4* d_rec = scratch_get<float4>(c, 15, (size_t)n);
    const bool side_scan = device_scan_side_ok((int)ncells);
    unsigned* d_sums = side_scan ? scratch_get<unsigned>(c, 16, device_scan_side_words((int)ncells)) : nullptr;
    if (!d_bx || !d_ba || !d_keys || !d_start || !d_cnt || !d_rec || (side_scan && !d_sums)) return ICPMI_ERR_HIP;
    if (!side_scan && stream != c->stream) { c->last_error = "dynamic_points_update: internal -- side stream with a table the two-kernel scan cannot take"; return ICPMI_ERR_UNSUPPORTED; }
    const Mat16 M = mat16(T);
    // counts -> starts in cursor layout (map_build.hip): one table to clear, the starts are written in full by the scan
    HIP_TRY(c, hipMemsetAsync(d_cnt, 0, ((size_t)ncells + 2) * sizeof(unsigned), stream));
    const int nb = (int)((n + 255) / 256), mb = (int)((m + 255) / 256);
    hipLaunchKernelGGL(dyn_beams_kernel, dim3(nb), dim3(256), 0, stream, d_in, n, M, g, d_bx, d_ba, d_keys, d_cnt);
    icpmi_status st = side_scan ? device_exclusive_scan_cursor_side(c, stream, d_sums, d_cnt, d_start, (int)ncells, (unsigned)n)
                                : device_exclusive_scan_cursor(c, d_cnt, d_start, (int)ncells, (unsigned)n, false);
    if (st != ICPMI_OK) return st;
    hipLaunchKernelGGL(dyn_scatter_kernel, dim3(nb), dim3(256), 0, stream, n, d_keys, d_start + 1, d_ba, d_rec);
    hipLaunchKernelGGL(dyn_update_kernel, dim3(mb), dim3(256), 0, stream, d_map, d_nrm, m, M, g, dp, (const float4*)d_bx, (const float4*)d_rec, (const unsigned*)d_start, d_prob);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// whether the side scan of dynpts_dev is available for these parameters (the chain asks before it forks)
bool dynpts_side_ok(const icpmi_dynpts_params* prm)
{
    DynGrid g;
    const int64_t ncells = dyn_grid(prm, g);
    return ncells <= DYN_MAX_CELLS && device_scan_side_ok((int)ncells);
}

// whether the module can run with these parameters at all: the map-update chain asks before it touches the resident map
icpmi_status dynpts_check(icpmi_ctx* c, const icpmi_dynpts_params* prm)
{
    DynGrid g;
    if (dyn_grid(prm, g) > DYN_MAX_CELLS) { c->last_error = "dynamic_points_update: beamHalfAngle too small for the angular grid"; return ICPMI_ERR_UNSUPPORTED; }
    return ICPMI_OK;
}

icpmi_status ops_dynamic_points_update(icpmi_ctx* c, const icpmi_dynpts_params* prm, const float to_sensor[16], const float* in4, int64_t n,
                                       const float* map4, const float* map_normals3, int64_t m, float* prob)
{
    if (n == 0 || m == 0) return ICPMI_OK;
    DevBuf<float> d_nrm, d_prob; DevBuf<float4> d_in, d_map;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_map.alloc((size_t)m));
    HIP_TRY(c, d_nrm.alloc((size_t)m * 3));
    HIP_TRY(c, d_prob.alloc((size_t)m));
    HIP_TRY(c, hipMemcpyAsync(d_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_map, map4, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_nrm, map_normals3, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_prob, prob, (size_t)m * sizeof(float), hipMemcpyHostToDevice, c->stream));
    icpmi_status st = dynpts_dev(c, prm, to_sensor, d_in, n, d_map, d_nrm, m, d_prob, c->stream);
    if (st != ICPMI_OK) return st;
    HIP_TRY(c, hipMemcpyAsync(prob, d_prob, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ICPMI_OK;
}
