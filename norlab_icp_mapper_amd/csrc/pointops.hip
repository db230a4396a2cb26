// pointops.hip -- the stateless operators on a caller's cloud (nothing here reads or writes a handle's resident map):
//   RigidTransformation::compute            (Mapper.cpp:197,221; Map.cpp:523,525)
//   SurfaceNormalDataPointsFilter           (Map.cpp:524 through examples/config.yaml:26-27)
//   PointDistanceMapperModule keep mask     (MapperModules/PointDistanceMapperModule.cpp:28-50)
//   Map::unloadCells cell binning           (Map.cpp:206-209,232-235)
//   the fused input filters, the fused sensor-model filters and the voxel sub-sample
// and the private-handle plumbing they search through (make_temp / temp_knn).  The operators on the resident map are in ops.hip, the
// DynamicPoints module in dynpts.hip.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void transform_kernel(const float4* __restrict__ in, int64_t n, Mat16 M, float4* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* T = M.v;
    const float4 p = in[i];
    const float3 o = xf_point(T, p.x, p.y, p.z, p.w);
    const float w = fmaf(T[15], p.w, fmaf(T[11], p.z, fmaf(T[7], p.y, T[3] * p.x)));
    out[i] = make_float4(o.x, o.y, o.z, w);
}

__global__ __launch_bounds__(256) void rotate3_kernel(const float* __restrict__ in3, int64_t n, Mat16 M, float* __restrict__ out3)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* T = M.v;
    const float x = in3[3 * i], y = in3[3 * i + 1], z = in3[3 * i + 2];
    out3[3 * i] = fmaf(T[8], z, fmaf(T[4], y, T[0] * x));
    out3[3 * i + 1] = fmaf(T[9], z, fmaf(T[5], y, T[1] * x));
    out3[3 * i + 2] = fmaf(T[10], z, fmaf(T[6], y, T[2] * x));
}

// RigidTransformation::compute on a whole resident cloud, in place: features by T and -- n3 != nullptr -- normals by its rotation, one
// launch (the arithmetic of transform_kernel and rotate3_kernel, element for element)
__global__ __launch_bounds__(256) void move_kernel(float4* __restrict__ pts, float* __restrict__ n3, int64_t n, Mat16 M)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* T = M.v;
    const float4 p = pts[i];
    const float3 o = xf_point(T, p.x, p.y, p.z, p.w);
    const float w = fmaf(T[15], p.w, fmaf(T[11], p.z, fmaf(T[7], p.y, T[3] * p.x)));
    pts[i] = make_float4(o.x, o.y, o.z, w);
    if (n3) {
        const float x = n3[3 * i], y = n3[3 * i + 1], z = n3[3 * i + 2];
        n3[3 * i] = fmaf(T[8], z, fmaf(T[4], y, T[0] * x));
        n3[3 * i + 1] = fmaf(T[9], z, fmaf(T[5], y, T[1] * x));
        n3[3 * i + 2] = fmaf(T[10], z, fmaf(T[6], y, T[2] * x));
    }
}

// ... out of place, normals always: a start of icpmi_voxel_register_multistart* into its slices, one launch (the same arithmetic again,
// element for element: the slices hold the bits icpmi_transform returns)
__global__ __launch_bounds__(256) void move_to_kernel(const float4* __restrict__ in, const float* __restrict__ in3, int64_t n, Mat16 M,
                                                      float4* __restrict__ out, float* __restrict__ out3)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* T = M.v;
    const float4 p = in[i];
    const float3 o = xf_point(T, p.x, p.y, p.z, p.w);
    const float w = fmaf(T[15], p.w, fmaf(T[11], p.z, fmaf(T[7], p.y, T[3] * p.x)));
    out[i] = make_float4(o.x, o.y, o.z, w);
    const float x = in3[3 * i], y = in3[3 * i + 1], z = in3[3 * i + 2];
    out3[3 * i] = fmaf(T[8], z, fmaf(T[4], y, T[0] * x));
    out3[3 * i + 1] = fmaf(T[9], z, fmaf(T[5], y, T[1] * x));
    out3[3 * i + 2] = fmaf(T[10], z, fmaf(T[6], y, T[2] * x));
}

__global__ __launch_bounds__(256) void bin_kernel(const float4* __restrict__ in, int64_t n, float cell, int* __restrict__ ijk)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    ijk[3 * i] = (int)floorf(p.x / cell);
    ijk[3 * i + 1] = (int)floorf(p.y / cell);
    ijk[3 * i + 2] = (int)floorf(p.z / cell);
}

__global__ __launch_bounds__(256) void keep_kernel(const float* __restrict__ d2, int64_t n, double lim, uint8_t* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = (double)d2[i] >= lim ? 1 : 0; // `dists(i) >= std::pow(minDistNewPoint, 2)`: a double comparison (PointDistanceMapperModule.cpp:42)
}

// one lane per point: mean + covariance of the kNN set in double, smallest eigenvector by Jacobi
// densities (may be null): `keepDensities` of the filter -- points per volume of the sphere that holds the neighbourhood around
// its centroid: k / (4/3 pi r^3), r = the largest distance of a neighbour from the centroid (computeDensity)
// mean_dist (may be null): `keepMeanDist` -- distance from the point to the mean of its neighbours.  The point is read as its own first
// neighbour (d2 = 0 sorts first; a duplicate that wins the index tie has the same coordinates), which keeps it in the index's centred frame.
// KMAX > 0 (k <= KMAX; r5): the row of neighbour ids and the k neighbours are requested up front -- two round trips -- and both passes (mean,
// scatter matrix) run from registers in the same order; the generic variant (KMAX = 0: any k) walks them one dependent load after the other,
// twice.  Same sums in the same order: same bits.
template <int KMAX>
__global__ __launch_bounds__(128) void normals_kernel(const float4* __restrict__ map, const int* __restrict__ sidx, int64_t m, int k,
                                                      float* __restrict__ normals3, float* __restrict__ densities, int dim2,
                                                      float* __restrict__ mean_dist = nullptr, float* __restrict__ eig_values = nullptr,
                                                      float* __restrict__ eig_vectors = nullptr, const unsigned* __restrict__ list = nullptr)
{
    // list (r6): an appended cloud -- m entries, the points whose neighbourhood was searched again (surface_normals_dev); otherwise all m points
    const int64_t t = (int64_t)blockIdx.x * 128 + threadIdx.x;
    if (t >= m) return;
    const int64_t i = list ? (int64_t)list[t] : t;
    // (r2: walking the points in cell-sorted order instead -- coherent neighbour gathers, scattered row reads and normal
    // writes -- measured 108 -> 164 us on the octree-ordered 0.9 M-point map and within noise on an append-ordered one: kept
    // in the caller's order)
    double mean[3] = {0, 0, 0};
    int real = 0;
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0, rmax2 = 0;
    float4 p0 = make_float4(0.f, 0.f, 0.f, 0.f); // the point itself (its own first neighbour), or map[0] where the row starts with "none"
    if constexpr (KMAX > 0) {
        int sv[KMAX];
        float4 qv[KMAX];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) sv[j] = j < k ? sidx[(size_t)k * i + j] : -1;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) qv[j] = map[sv[j] < 0 ? 0 : sv[j]];
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (sv[j] >= 0) { mean[0] += qv[j].x; mean[1] += qv[j].y; mean[2] += qv[j].z; ++real; }
        const double inv = 1.0 / (real > 0 ? real : 1);
        mean[0] *= inv; mean[1] *= inv; mean[2] *= inv;
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (sv[j] >= 0) {
                const double x = qv[j].x - mean[0], y = qv[j].y - mean[1], z = qv[j].z - mean[2];
                c00 += x * x; c01 += x * y; c02 += x * z; c11 += y * y; c12 += y * z; c22 += z * z;
                const double r2 = x * x + y * y + z * z;
                rmax2 = r2 > rmax2 ? r2 : rmax2;
            }
        p0 = qv[0];
    } else {
        for (int j = 0; j < k; ++j) {
            const int s = sidx[(size_t)k * i + j];
            if (s < 0) continue;
            const float4 q = map[s];
            mean[0] += q.x; mean[1] += q.y; mean[2] += q.z; ++real;
        }
        const double inv = 1.0 / (real > 0 ? real : 1);
        mean[0] *= inv; mean[1] *= inv; mean[2] *= inv;
        for (int j = 0; j < k; ++j) {
            const int s = sidx[(size_t)k * i + j];
            if (s < 0) continue;
            const float4 q = map[s];
            const double x = q.x - mean[0], y = q.y - mean[1], z = q.z - mean[2];
            c00 += x * x; c01 += x * y; c02 += x * z; c11 += y * y; c12 += y * z; c22 += z * z;
            const double r2 = x * x + y * y + z * z;
            rmax2 = r2 > rmax2 ? r2 : rmax2;
        }
        if (mean_dist) { const int s0 = sidx[(size_t)k * i]; p0 = map[s0 < 0 ? 0 : s0]; }
    }
    if (densities) {
        const double r = sqrt(rmax2);
        densities[i] = (float)((double)real / ((4.0 / 3.0) * 3.14159265358979323846 * (r * r * r)));
    }
    if (mean_dist) {
        const double x = p0.x - mean[0], y = p0.y - mean[1], z = p0.z - mean[2];
        mean_dist[i] = (float)sqrt(x * x + y * y + z * z);
    }
    // cyclic Jacobi on the symmetric 3x3
    double A[3][3] = {{c00, c01, c02}, {c01, c11, c12}, {c02, c12, c22}};
    double Q[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dg = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (off <= 1e-32 * dg || off < 1e-300) break;
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) {
                    const double akp = A[kk][p], akq = A[kk][q];
                    A[kk][p] = c * akp - s * akq; A[kk][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) {
                    const double apk = A[p][kk], aqk = A[q][kk];
                    A[p][kk] = c * apk - s * aqk; A[q][kk] = s * apk + c * aqk;
                }
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) {
                    const double qkp = Q[kk][p], qkq = Q[kk][q];
                    Q[kk][p] = c * qkp - s * qkq; Q[kk][q] = s * qkp + c * qkq;
                }
            }
    }
    const double w0 = A[0][0], w1 = A[1][1], w2 = A[2][2];
    const double wmax = fmax(fabs(w0), fmax(fabs(w1), fabs(w2)));
    const double thr = 3.0 * 1.1920928955078125e-07 * wmax;
    const int rank = (wmax > 0) ? ((fabs(w0) > thr) + (fabs(w1) > thr) + (fabs(w2) > thr)) : 0;
    if ((eig_values || eig_vectors) && !dim2) {
        // keepEigenValues / keepEigenVectors with sortEigen: 1 (r5): eigenvalues of the scatter matrix ascending (the exchange sort (0,1) (0,2)
        // (1,2), strict), serializeEigVec of the eigenvector matrix in that column order -- entry 3 k + j = component k of eigenvector j;
        // rank < 2: upstream's degenerate answer (zeros, identity).  Static indices only (no scratch).
        double e0 = w0, e1 = w1, e2 = w2;
        int o0 = 0, o1 = 1, o2 = 2;
        if (rank >= 2) {
            if (e1 < e0) { const double t = e0; e0 = e1; e1 = t; const int u = o0; o0 = o1; o1 = u; }
            if (e2 < e0) { const double t = e0; e0 = e2; e2 = t; const int u = o0; o0 = o2; o2 = u; }
            if (e2 < e1) { const double t = e1; e1 = e2; e2 = t; const int u = o1; o1 = o2; o2 = u; }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int oj = j == 0 ? o0 : (j == 1 ? o1 : o2);
            const double wj = j == 0 ? e0 : (j == 1 ? e1 : e2);
            if (eig_values) eig_values[3 * i + j] = rank >= 2 ? (float)wj : 0.f;
            if (eig_vectors) {
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) {
                    const double q = oj == 0 ? Q[kk][0] : (oj == 1 ? Q[kk][1] : Q[kk][2]);
                    eig_vectors[9 * i + 3 * kk + j] = rank >= 2 ? (float)q : (kk == j ? 1.f : 0.f);
                }
            }
        }
    }
    float nx = 1.f, ny = 0.f, nz = 0.f; // upstream's degenerate answer: eigenvectors = identity
    if (dim2) {
        // planar cloud (z == 0: the rotations with the z axis saw zero off-diagonals): the smaller eigenvector of the plane's pair;
        // upstream needs rank + 1 >= featDim - 1 = 2 there, i.e. rank >= 1
        const double wm2 = fmax(fabs(w0), fabs(w1));
        const double thr2 = 2.0 * 1.1920928955078125e-07 * wm2;
        const int rank2 = (wm2 > 0) ? ((fabs(w0) > thr2) + (fabs(w1) > thr2)) : 0;
        if (rank2 >= 1) {
            const int e2 = w1 < w0 ? 1 : 0;
            nx = (float)(e2 == 0 ? Q[0][0] : Q[0][1]);
            ny = (float)(e2 == 0 ? Q[1][0] : Q[1][1]);
            nz = 0.f;
        }
    } else if (rank >= 2) {
        int e = 0;
        double wm = w0;
        if (w1 < wm) { wm = w1; e = 1; }
        if (w2 < wm) { wm = w2; e = 2; }
        nx = (float)(e == 0 ? Q[0][0] : (e == 1 ? Q[0][1] : Q[0][2]));
        ny = (float)(e == 0 ? Q[1][0] : (e == 1 ? Q[1][1] : Q[1][2]));
        nz = (float)(e == 0 ? Q[2][0] : (e == 1 ? Q[2][1] : Q[2][2]));
    }
    normals3[3 * i] = nx; normals3[3 * i + 1] = ny; normals3[3 * i + 2] = nz;
}

// ---- intensity gradients of a cloud with normals (icpmi_intensity_gradient / icpmi_set_map_intensity) ----
// the intensities in the order of the search index: position s of `sorted` holds the cloud's point float_as_uint(sorted[s].w), whose
// intensity is inten[that index] -- or, iperm != nullptr (the resident map: the cloud is the registration index's sorted array, the row is
// in the caller's order), inten[float_as_uint(iperm[that index].w)]
__global__ __launch_bounds__(256) void intensity_gather_kernel(const float4* __restrict__ sorted, int64_t m, const float* __restrict__ inten,
                                                               const float4* __restrict__ iperm, float* __restrict__ out)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x; s < m; s += stride) {
        unsigned o = __float_as_uint(sorted[s].w);
        if (iperm && o < (unsigned)m) o = __float_as_uint(iperm[o].w);
        out[s] = o < (unsigned)m ? inten[o] : NAN; // (an index past the row: never for a cloud the search built; NaN = no intensity)
    }
}

// One lane per point of the cloud, grid-stride: the least-squares gradient of the intensity over its K = k - 1 nearest other points, in the
// tangent plane of its normal.  rows of sidx: the cloud's order, entries = positions in `sorted` (-1: unfilled), the point itself (or a
// duplicate of it) first; isorted: intensity_gather_kernel's row.  nrm: the normals in the cloud's order, nstride floats apart.  Float
// arithmetic in neighbour order, no atomics: the same bits on every call.  The neighbour ids of a chunk are requested together, then their
// points and intensities: two round trips per CH neighbours.
// Out: grad3 (3 floats per point) and / or gi4 = (g.x, g.y, g.z, I) per point.
__global__ __launch_bounds__(256) void intensity_gradient_kernel(const float4* __restrict__ sorted, const int* __restrict__ sidx, const float* __restrict__ isorted,
                                                                 const float* __restrict__ nrm, int nstride, const float* __restrict__ inten,
                                                                 const float4* __restrict__ iperm, int64_t m, int k, float* __restrict__ grad3,
                                                                 float4* __restrict__ gi4)
{
    constexpr int CH = 8;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
        const int* row = sidx + (size_t)k * i;
        const int s0 = row[0];
        const float nx = nrm[(size_t)nstride * i], ny = nrm[(size_t)nstride * i + 1], nz = nrm[(size_t)nstride * i + 2];
        unsigned io = (unsigned)i;
        if (iperm) io = __float_as_uint(iperm[i].w);
        const float Ii = io < (unsigned)m ? inten[io] : NAN;
        const float4 xi = sorted[s0 < 0 ? 0 : s0];
        // u = n / |n|; a zero or non-finite normal has no tangent plane
        const float l2 = nx * nx + ny * ny + nz * nz;
        const bool ok = s0 >= 0 && l2 > 0.f && l2 < INFINITY && fabsf(Ii) < INFINITY;
        const float inv = 1.f / sqrtf(ok ? l2 : 1.f);
        const float ux = nx * inv, uy = ny * inv, uz = nz * inv;
        // e1 = normalise(u x axis), axis = the coordinate axis of the smallest |u| component (the first of equals); e2 = u x e1
        const float ax = fabsf(ux), ay = fabsf(uy), az = fabsf(uz);
        float cx, cy, cz;
        if (ax <= ay && ax <= az) { cx = 0.f; cy = uz; cz = -uy; }
        else if (ay <= az) { cx = -uz; cy = 0.f; cz = ux; }
        else { cx = uy; cy = -ux; cz = 0.f; }
        const float cinv = 1.f / sqrtf(cx * cx + cy * cy + cz * cz);
        const float e1x = cx * cinv, e1y = cy * cinv, e1z = cz * cinv;
        const float e2x = uy * e1z - uz * e1y, e2y = uz * e1x - ux * e1z, e2z = ux * e1y - uy * e1x;
        float saa = 0.f, sab = 0.f, sbb = 0.f, ra = 0.f, rb = 0.f;
        int used = 0;
        for (int j0 = 1; j0 < k && ok; j0 += CH) {
            int sv[CH]; float4 xv[CH]; float iv[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j) sv[j] = j0 + j < k ? row[j0 + j] : -1;
#pragma unroll
            for (int j = 0; j < CH; ++j) { xv[j] = sorted[sv[j] < 0 ? 0 : sv[j]]; iv[j] = isorted[sv[j] < 0 ? 0 : sv[j]]; }
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (sv[j] < 0 || !(fabsf(iv[j]) < INFINITY)) continue; // unfilled slot; a neighbour without an intensity
                const float dx = xv[j].x - xi.x, dy = xv[j].y - xi.y, dz = xv[j].z - xi.z;
                const float t = dx * ux + dy * uy + dz * uz;
                const float px = dx - ux * t, py = dy - uy * t, pz = dz - uz * t;
                const float a = px * e1x + py * e1y + pz * e1z, b = px * e2x + py * e2y + pz * e2z;
                const float dI = iv[j] - Ii;
                saa += a * a; sab += a * b; sbb += b * b;
                ra += a * dI; rb += b * dI;
                ++used;
            }
        }
        // g2 = S^-1 r in closed form; neighbours on a line or on the point itself (det S <= 1e-4 (tr S / 2)^2) give no gradient
        const float det = saa * sbb - sab * sab, htr = (saa + sbb) * 0.5f;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (ok && used >= 2 && det > 1e-4f * (htr * htr)) {
            const float g2x = (sbb * ra - sab * rb) / det, g2y = (saa * rb - sab * ra) / det;
            gx = g2x * e1x + g2y * e2x; gy = g2x * e1y + g2y * e2y; gz = g2x * e1z + g2y * e2z;
        }
        if (grad3) { grad3[3 * i] = gx; grad3[3 * i + 1] = gy; grad3[3 * i + 2] = gz; }
        if (gi4) gi4[i] = make_float4(gx, gy, gz, Ii);
    }
}

} // namespace

// k <= 10 (the shipped SurfaceNormalDataPointsFilter{knn: 10}) and k <= 16 keep the neighbourhood in registers; ICPMI_NORMALS_REG=0: the generic walk
void launch_normals(hipStream_t stream, const float4* map, const int* sidx, int64_t m, int k, float* normals3, float* densities, int dim2,
                    float* mean_dist, float* eig_values, float* eig_vectors, const unsigned* list)
{
    constexpr int reg = 1;
    const dim3 grid((int)((m + 127) / 128)), block(128);
    if (reg && k <= 10) hipLaunchKernelGGL(normals_kernel<10>, grid, block, 0, stream, map, sidx, m, k, normals3, densities, dim2, mean_dist, eig_values, eig_vectors, list);
    else if (reg && k <= 16) hipLaunchKernelGGL(normals_kernel<16>, grid, block, 0, stream, map, sidx, m, k, normals3, densities, dim2, mean_dist, eig_values, eig_vectors, list);
    else hipLaunchKernelGGL(normals_kernel<0>, grid, block, 0, stream, map, sidx, m, k, normals3, densities, dim2, mean_dist, eig_values, eig_vectors, list);
}

namespace {

// ---- fused input filters (Mapper::applyInputFilters): one predicate pass for a run of DistanceLimit / BoundingBox filters ----
struct FilterPack { icpmi_point_filter f[ICPMI_MAX_POINT_FILTERS]; int n; };

__global__ __launch_bounds__(256) void filter_points_kernel(const float4* __restrict__ in, int64_t n, FilterPack fp, uint8_t* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    bool ok = true;
    for (int k = 0; k < fp.n; ++k) {
        const icpmi_point_filter& f = fp.f[k];
        if (f.type == ICPMI_FILT_DISTANCE_LIMIT) {
            // sqrtf of the sum in the oracle's order (no contraction: -ffp-contract=off on both sides)
            const float v = f.i < 0 ? sqrtf(p.x * p.x + p.y * p.y + p.z * p.z) : fabsf(f.i == 0 ? p.x : (f.i == 1 ? p.y : p.z));
            const float ad = fabsf(f.f[0]);
            ok &= f.f[1] != 0.f ? v > ad : v < ad;
        } else {
            const bool inside = p.x > f.f[0] && p.x < f.f[3] && p.y > f.f[1] && p.y < f.f[4] && p.z > f.f[2] && p.z < f.f[5];
            ok &= f.i ? !inside : inside;
        }
    }
    keep[i] = ok ? 1 : 0;
}

// ---- fused sensor-model filters (include/icpmi.h: icpmi_sensor_model): ObservationDirection / OrientNormals / Shadow /
// SimpleSensorNoise as one program per point; od, n, keep and noise stay in registers across the steps ----
struct SensorPack {
    icpmi_sensor_step s[ICPMI_MAX_SENSOR_STEPS]; int n;
    int read_n, write_n, read_od, write_od; // which of the in/out rows the program touches
};

// n3 / od3 are read and written in place by the thread that owns the point (no __restrict__: the same buffer both ways).
// No contraction (-ffp-contract=off): every product, sum, division and sqrtf below is one correctly rounded float32 operation.
__global__ __launch_bounds__(256) void sensor_model_kernel(const float4* __restrict__ in, int64_t n, SensorPack sp, float* n3, float* od3,
                                                           float* __restrict__ noise_out, uint8_t* __restrict__ keep_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    float nx = 0.f, ny = 0.f, nz = 0.f, ox = 0.f, oy = 0.f, oz = 0.f, noise = 0.f;
    if (sp.read_n) { nx = n3[3 * i]; ny = n3[3 * i + 1]; nz = n3[3 * i + 2]; }
    if (sp.read_od) { ox = od3[3 * i]; oy = od3[3 * i + 1]; oz = od3[3 * i + 2]; }
    bool keep = true;
    for (int k = 0; k < sp.n; ++k) {
        const icpmi_sensor_step& s = sp.s[k];
        if (s.type == ICPMI_SM_OBSERVATION_DIRECTION) {
            ox = s.f[0] - p.x; oy = s.f[1] - p.y; oz = s.f[2] - p.z;
        } else if (s.type == ICPMI_SM_ORIENT_NORMALS) {
            const float d = nx * ox + ny * oy + nz * oz;
            if (s.i ? d < 0.f : d > 0.f) { nx = -nx; ny = -ny; nz = -nz; }
        } else if (s.type == ICPMI_SM_SHADOW) {
            const float ln = sqrtf(nx * nx + ny * ny + nz * nz), lp = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z);
            const float v = fabsf((nx / ln) * (p.x / lp) + (ny / ln) * (p.y / lp) + (nz / ln) * (p.z / lp));
            keep = keep && v > s.f[0]; // (a NaN compares false: dropped)
        } else {
            const float dist = sqrtf(p.x * p.x + p.y * p.y + p.z * p.z), gain = s.f[0];
            if (s.i <= 2) {
                const float min_radius = s.i == 0 ? 0.012f : (s.i == 1 ? 0.028f : 0.018f);
                const float beam_angle = s.i == 0 ? 0.0068f : (s.i == 1 ? 0.0013f : 0.0006f);
                const float beam_const = s.i == 0 ? 0.0008f : (s.i == 1 ? 0.0001f : 0.0015f);
                const float t = beam_angle * dist + beam_const;
                noise = gain * (t > min_radius ? t : min_radius);
            } else {
                noise = ((gain * 0.5f) * 0.00285f) * (dist * dist);
            }
        }
    }
    if (sp.write_n) { n3[3 * i] = nx; n3[3 * i + 1] = ny; n3[3 * i + 2] = nz; }
    if (sp.write_od) { od3[3 * i] = ox; od3[3 * i + 1] = oy; od3[3 * i + 2] = oz; }
    if (noise_out) noise_out[i] = noise;
    if (keep_out) keep_out[i] = keep ? 1 : 0;
}

// ---- voxel sub-sample (OctreeMapperModule / OctreeGridDataPointsFilter stand-in, samplingMethod 0) ----
// lattice anchored at the bounding-box minimum; voxel index floor((p - lo) / edge) per axis, 21 bits
// each; the representative of a voxel is its point of smallest original index (order independent:
// atomicMin), so the keep mask is a function of the input alone.
__global__ __launch_bounds__(256) void bbox_min_kernel(const float4* __restrict__ in, int64_t n, unsigned* __restrict__ lo_keys)
{
    __shared__ unsigned sh[3][4];
    unsigned kx = 0xffffffffu, ky = 0xffffffffu, kz = 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float4 p = in[i];
        kx = min(kx, float_key(p.x)); ky = min(ky, float_key(p.y)); kz = min(kz, float_key(p.z));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kx = min(kx, (unsigned)__shfl_xor((int)kx, off, 64));
        ky = min(ky, (unsigned)__shfl_xor((int)ky, off, 64));
        kz = min(kz, (unsigned)__shfl_xor((int)kz, off, 64));
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { sh[0][w] = kx; sh[1][w] = ky; sh[2][w] = kz; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned v = min(min(sh[threadIdx.x][0], sh[threadIdx.x][1]), min(sh[threadIdx.x][2], sh[threadIdx.x][3]));
        atomicMin(&lo_keys[threadIdx.x], v);
    }
}

__device__ __forceinline__ unsigned long long voxel_key(const float4 p, const unsigned* __restrict__ lo_keys, float edge)
{
    const float lo[3] = {float_key_inv(lo_keys[0]), float_key_inv(lo_keys[1]), float_key_inv(lo_keys[2])};
    const float c[3] = {p.x, p.y, p.z};
    unsigned long long key = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float v = fminf(floorf((c[r] - lo[r]) / edge), 2097151.0f);
        key = key * 2097152ull + (unsigned long long)v;
    }
    return key;
}

__global__ __launch_bounds__(256) void voxel_insert_kernel(const float4* __restrict__ in, int64_t n, const unsigned* __restrict__ lo_keys,
                                                           float edge, int method, unsigned long long* __restrict__ tkeys,
                                                           unsigned* __restrict__ tvals, unsigned long long mask,
                                                           unsigned* __restrict__ slot_of)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = voxel_key(in[i], lo_keys, edge);
    unsigned long long slot = mix64(key) & mask;
    for (;;) {
        const unsigned long long prev = atomicCAS(&tkeys[slot], ~0ull, key);
        if (prev == ~0ull || prev == key) break;
        slot = (slot + 1) & mask;
    }
    atomicMin(&tvals[slot], method ? fmix32((unsigned)i) : (unsigned)i);
    slot_of[i] = (unsigned)slot;
}

// flag[i] = 1 iff i represents its voxel (T = uint8_t for the host mask, unsigned for device compaction)
template <typename T>
__global__ __launch_bounds__(256) void voxel_keep_kernel(int64_t n, const unsigned* __restrict__ tvals, const unsigned* __restrict__ slot_of,
                                                         int method, T* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = tvals[slot_of[i]] == (method ? fmix32((unsigned)i) : (unsigned)i) ? 1 : 0;
}
} // namespace

// private handles enqueue on the owner's stream: what they read was produced there and what they produce is consumed there,
// so stream order replaces the hipStreamSynchronize pairs an own stream needs (r2: two per surface-normal step of a map update)
void share_stream(icpmi_ctx* c, icpmi_ctx* t)
{
    if (t->stream == c->stream) { (void)zero_state_if_pending(t); return; } // (a handle that keeps its own stream still starts from a cleared state: ADVICE r5)
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    if (t->own_stream && t->stream) stream_release(t->stream);
    t->stream = c->stream; t->own_stream = false;
    drop_loop_graphs(t);
    (void)zero_state_if_pending(t); // (on the owner's stream; an error surfaces at the handle's next call)
}

icpmi_status make_temp(icpmi_ctx* c, TempCtx& t)
{
    if (!c->temp) {
        icpmi_config cfg = c->cfg;
        icpmi_status s = create_handle(&cfg, &c->temp);
        if (s != ICPMI_OK) { c->last_error = icpmi_last_error(nullptr); c->temp = nullptr; return s; }
    }
    t.h = c->temp;
    share_stream(c, t.h);
    t.h->cfg = c->cfg;
    t.h->keep_raw = false;
    t.h->no_centre = true; // PointDistanceMapperModule.cpp:33 / SurfaceNormalDataPointsFilter build their kd-tree on the raw cloud
    t.h->single_level = false;
    return ICPMI_OK;
}

// Transformation::checkParameters: rotation part must be (close to) orthonormal with det +1
icpmi_status check_rigid(icpmi_ctx* c, const float T[16])
{
    const double det = (double)T[0] * ((double)T[5] * T[10] - (double)T[9] * T[6]) - (double)T[4] * ((double)T[1] * T[10] - (double)T[9] * T[2]) +
                       (double)T[8] * ((double)T[1] * T[6] - (double)T[5] * T[2]);
    if (fabs(1.0 - det) > 1e-3) {
        c->last_error = "TransformationError: RigidTransformation: rotation part is not orthonormal (|1 - det| > 1e-3)";
        return ICPMI_ERR_INVALID_ARG;
    }
    return ICPMI_OK;
}

// RigidTransformation::compute on a whole device cloud in place: features by T, normals (d_n3 may be null) by its rotation (Map.cpp:523 / :525)
icpmi_status ops_move_dev(icpmi_ctx* c, const float T[16], float4* d_pts, float* d_n3, int64_t m)
{
    if (m == 0) return ICPMI_OK;
    const icpmi_status s = check_rigid(c, T);
    if (s != ICPMI_OK) return s;
    hipLaunchKernelGGL(move_kernel, dim3((int)((m + 255) / 256)), dim3(256), 0, c->stream, d_pts, d_n3, m, mat16(T));
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// RigidTransformation::compute on device buffers, on the handle's stream (the 4x4 goes through a small resident buffer)
icpmi_status ops_transform_dev(icpmi_ctx* c, const float T[16], const float4* d_in, int64_t n, float4* d_out)
{
    icpmi_status s = check_rigid(c, T);
    if (s != ICPMI_OK || n == 0) return s;
    hipLaunchKernelGGL(transform_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, n, mat16(T), d_out);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

// ... points and normals (3 floats per point) by T into buffers of the caller's, one launch; T passed check_rigid
icpmi_status ops_transform_normals_dev(icpmi_ctx* c, const float T[16], const float4* d_in, const float* d_in3, int64_t n, float4* d_out, float* d_out3)
{
    if (n == 0) return ICPMI_OK;
    hipLaunchKernelGGL(move_to_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, d_in3, n, mat16(T), d_out, d_out3);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

icpmi_status ops_transform(icpmi_ctx* c, const float T[16], const float* in4, int64_t n, float* out4, const float* in_n3,
                           float* out_n3)
{
    icpmi_status cs = check_rigid(c, T);
    if (cs != ICPMI_OK) return cs;
    if (n == 0) return ICPMI_OK;
    DevBuf<float> d_n, d_no;
    DevBuf<float4> d_in, d_out;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_out.alloc((size_t)n));
    hipError_t e = hipMemcpyAsync(d_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    const int blocks = (int)((n + 255) / 256);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(transform_kernel, dim3(blocks), dim3(256), 0, c->stream, d_in, n, mat16(T), d_out);
        e = hipMemcpyAsync(out4, d_out, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess && in_n3 && out_n3) {
        e = d_n.alloc((size_t)n * 3);
        if (e == hipSuccess) e = d_no.alloc((size_t)n * 3);
        if (e == hipSuccess) e = hipMemcpyAsync(d_n, in_n3, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(rotate3_kernel, dim3(blocks), dim3(256), 0, c->stream, d_n, n, mat16(T), d_no);
            e = hipMemcpyAsync(out_n3, d_no, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIP_TRY(c, e);
    return ICPMI_OK;
}

icpmi_status ops_bin_cells(icpmi_ctx* c, const float* pts4, int64_t n, float cell_size, int32_t* ijk3)
{
    if (n == 0) return ICPMI_OK;
    DevBuf<float4> d_in; DevBuf<int> d_o;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_o.alloc((size_t)n * 3));
    hipError_t e = hipMemcpyAsync(d_in, pts4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(bin_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, d_in, n, cell_size, d_o);
        e = hipMemcpyAsync(ijk3, d_o, (size_t)n * 3 * sizeof(int), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    HIP_TRY(c, e);
    return ICPMI_OK;
}

// shared by surface normals and point-distance: index `cloud4` in a temp handle, kNN `q4` against it
static icpmi_status temp_knn(icpmi_ctx* c, TempCtx& t, const float* cloud4, int64_t m, const float* q4, int64_t n, int k,
                             int allow_self, bool queries_are_cloud)
{
    icpmi_ctx* tc = t.h;
    const bool self = queries_are_cloud && allow_self; // SurfaceNormalDataPointsFilter: the cloud against itself -- the sparse block grid (selfgrid.hip)
    if (self) {
        if (m <= 0 || !cloud4) { c->last_error = "set_map: empty cloud"; return ICPMI_ERR_INVALID_ARG; }
        const size_t cnt = (size_t)m * k + 1;
        if (tc->d_stage_in.ensure(tc, (size_t)m + 1) != ICPMI_OK || tc->d_sidx.ensure(tc, cnt) != ICPMI_OK ||
            tc->d_d2.ensure(tc, cnt) != ICPMI_OK) { c->last_error = tc->last_error; return ICPMI_ERR_HIP; }
        HIP_TRY(c, hipMemcpyAsync(tc->d_stage_in, cloud4, (size_t)m * sizeof(float4), hipMemcpyHostToDevice, tc->stream));
        const icpmi_status gs = selfgrid_knn(tc, tc->d_stage_in, m, k, tc->d_sidx, tc->d_d2);
        if (gs != ICPMI_OK) c->last_error = tc->last_error;
        return gs;
    }
    tc->single_level = false;
    int32_t acc = 0;
    icpmi_status s = icpmi_set_map(t.h, cloud4, m, nullptr, &acc);
    if (s != ICPMI_OK) { c->last_error = tc->last_error; return s; }
    // queries: stage + centre on the temp map's mean (the index lives in the centred frame)
    // (the cloud itself is already there: icpmi_set_map staged it in d_stage_in -- no second upload, and no re-sizing
    // of that buffer, which would drop it)
    if (!queries_are_cloud) {
        if (tc->d_stage_in.ensure(tc, (size_t)n + 1) != ICPMI_OK) { c->last_error = tc->last_error; return ICPMI_ERR_HIP; }
        HIP_TRY(c, hipMemcpyAsync(tc->d_stage_in, q4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, tc->stream));
    }
    s = loop_prepare_reading(tc, tc->d_stage_in, n, nullptr);
    if (s != ICPMI_OK) { c->last_error = tc->last_error; return s; }
    LoopCfg lc = make_loop_cfg(tc, 1);
    lc.k = k; lc.max_dist = INFINITY; lc.maxr2 = INFINITY; lc.ring_max = 6; lc.inv1e = 1.f; lc.err2 = 1.f; // (a filter's search: exact whatever the matcher's epsilon)
    const size_t cnt = (size_t)n * k + 1;
    if (tc->d_sidx.ensure(tc, cnt) != ICPMI_OK || tc->d_d2.ensure(tc, cnt) != ICPMI_OK ||
        tc->d_hard.ensure(tc, (size_t)n + 1) != ICPMI_OK) { c->last_error = tc->last_error; return ICPMI_ERR_HIP; }
    HIP_TRY(c, hipMemsetAsync(tc->d_state, 0, sizeof(IcpState), tc->stream));
    s = nn_launch_k(tc, NnRequest(), tc->d_reading, n, nullptr, lc, allow_self, tc->d_sidx, tc->d_d2, tc->d_state);
    if (s != ICPMI_OK) { c->last_error = tc->last_error; return s; }
    return ICPMI_OK;
}

icpmi_status ops_surface_normals(icpmi_ctx* c, const float* pts4, int64_t m, int knn, float* normals3, float* densities, int32_t* matched_ids,
                                 float* mean_dist, float* eig_values, float* eig_vectors)
{
    if (m == 0) return ICPMI_OK;
    if (knn < 1 || knn > ICPMI_MAX_K) { c->last_error = "surface_normals: knn must be in [1, 32]"; return ICPMI_ERR_INVALID_ARG; }
    TempCtx t;
    icpmi_status s = make_temp(c, t);
    if (s != ICPMI_OK) return s;
    s = temp_knn(c, t, pts4, m, nullptr, m, knn, 1, true);
    if (s != ICPMI_OK) return s;
    icpmi_ctx* tc = t.h;
    if ((eig_values || eig_vectors) && c->cfg.is_2d) { c->last_error = "surface_normals: keepEigenValues / keepEigenVectors are not served for planar clouds"; return ICPMI_ERR_UNSUPPORTED; }
    DevBuf<float> d_n, d_dens, d_md, d_ev, d_evec;
    DevBuf<int> d_ids;
    HIP_TRY(c, d_n.alloc((size_t)m * 3));
    if (densities) HIP_TRY(c, d_dens.alloc((size_t)m));
    if (mean_dist) HIP_TRY(c, d_md.alloc((size_t)m));
    if (eig_values) HIP_TRY(c, d_ev.alloc((size_t)m * 3));
    if (eig_vectors) HIP_TRY(c, d_evec.alloc((size_t)m * 9));
    launch_normals(tc->stream, tc->d_map_sorted, tc->d_sidx, m, knn, d_n, densities ? d_dens.get() : (float*)nullptr, c->cfg.is_2d,
                   mean_dist ? d_md.get() : (float*)nullptr, eig_values ? d_ev.get() : (float*)nullptr, eig_vectors ? d_evec.get() : (float*)nullptr);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && eig_values) e = hipMemcpyAsync(eig_values, d_ev, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, tc->stream);
    if (e == hipSuccess && eig_vectors) e = hipMemcpyAsync(eig_vectors, d_evec, (size_t)m * 9 * sizeof(float), hipMemcpyDeviceToHost, tc->stream);
    if (e == hipSuccess && matched_ids) { // keepMatchedIds: sorted positions -> the caller's indices
        e = d_ids.alloc((size_t)m * knn);
        if (e == hipSuccess && nn_ids_to_original(tc, tc->d_sidx, m * knn, d_ids) != ICPMI_OK) { c->last_error = tc->last_error; return ICPMI_ERR_HIP; }
        if (e == hipSuccess) e = hipMemcpyAsync(matched_ids, d_ids, (size_t)m * knn * sizeof(int), hipMemcpyDeviceToHost, tc->stream);
    }
    if (e == hipSuccess && mean_dist) e = hipMemcpyAsync(mean_dist, d_md, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, tc->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(normals3, d_n, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, tc->stream);
    if (e == hipSuccess && densities) e = hipMemcpyAsync(densities, d_dens, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, tc->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(tc->stream);
    HIP_TRY(c, e);
    return ICPMI_OK;
}

// workgroups of the two intensity kernels: one lane per point up to 2048 workgroups, a grid-stride walk past that
static int intensity_grid(int64_t m) { const int64_t nb = (m + 255) / 256; return (int)(nb > 2048 ? 2048 : nb); }

// the gradient pass behind a self search of the private handle tc over a cloud of m points with k = knn + 1 (rows in tc->d_sidx, the search's
// order in tc->d_map_sorted): d_nrm / nstride, d_inten, iperm as intensity_gradient_kernel takes them; d_isorted: m floats of scratch
static void launch_intensity_gradient(icpmi_ctx* tc, int64_t m, int k, const float* d_nrm, int nstride, const float* d_inten, const float4* iperm,
                                      float* d_isorted, float* d_grad3, float4* d_gi4)
{
    const int nb = intensity_grid(m);
    hipLaunchKernelGGL(intensity_gather_kernel, dim3(nb), dim3(256), 0, tc->stream, (const float4*)tc->d_map_sorted, m, d_inten, iperm, d_isorted);
    hipLaunchKernelGGL(intensity_gradient_kernel, dim3(nb), dim3(256), 0, tc->stream, (const float4*)tc->d_map_sorted, (const int*)tc->d_sidx,
                       (const float*)d_isorted, d_nrm, nstride, d_inten, iperm, m, k, d_grad3, d_gi4);
}

// icpmi_intensity_gradient: the operator on host pointers -- the self search of ops_surface_normals with k = knn + 1, then the gradient pass
icpmi_status ops_intensity_gradient(icpmi_ctx* c, const float* pts4, int64_t m, const float* normals3, const float* intensity, int knn, float* grad3)
{
    if (m == 0) return ICPMI_OK;
    if (knn < 1 || knn > ICPMI_MAX_K - 1) { c->last_error = "intensity_gradient: knn must be in [1, 31]"; return ICPMI_ERR_INVALID_ARG; }
    TempCtx t;
    icpmi_status s = make_temp(c, t);
    if (s != ICPMI_OK) return s;
    c->dk_m = 0; // (the private handle's grid is searched over another cloud: the k-th distances remembered for the resident map's next append are gone)
    s = temp_knn(c, t, pts4, m, nullptr, m, knn + 1, 1, true);
    if (s != ICPMI_OK) return s;
    icpmi_ctx* tc = t.h;
    DevBuf<float> d_n, d_i, d_is, d_g;
    HIP_TRY(c, d_n.alloc((size_t)m * 3));
    HIP_TRY(c, d_i.alloc((size_t)m));
    HIP_TRY(c, d_is.alloc((size_t)m));
    HIP_TRY(c, d_g.alloc((size_t)m * 3));
    HIP_TRY(c, hipMemcpyAsync(d_n, normals3, (size_t)m * 3 * sizeof(float), hipMemcpyHostToDevice, tc->stream));
    HIP_TRY(c, hipMemcpyAsync(d_i, intensity, (size_t)m * sizeof(float), hipMemcpyHostToDevice, tc->stream));
    launch_intensity_gradient(tc, m, knn + 1, d_n, 3, d_i, nullptr, d_is, d_g, nullptr);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(grad3, d_g, (size_t)m * 3 * sizeof(float), hipMemcpyDeviceToHost, tc->stream));
    HIP_TRY(c, hipStreamSynchronize(tc->stream));
    return ICPMI_OK;
}

// icpmi_set_map_intensity: the same two kernels over the resident map AS THE INDEX HOLDS IT -- the cloud is c->d_map_sorted (a gradient does
// not see the centring), its normals c->d_normals_sorted, so the (g, I) row comes out in the index's order, the way the normals are kept; the
// caller's row is read through the original index in every sorted point's w.  The caller has checked m == c->m and the normals.
icpmi_status ops_set_map_intensity(icpmi_ctx* c, const float* intensity, int64_t m, int knn)
{
    if (knn < 1 || knn > ICPMI_MAX_K - 1) { c->last_error = "set_map_intensity: knn must be in [1, 31]"; return ICPMI_ERR_INVALID_ARG; }
    c->gi_m = 0;
    TempCtx t;
    icpmi_status s = make_temp(c, t);
    if (s != ICPMI_OK) return s;
    icpmi_ctx* tc = t.h;
    const int k = knn + 1;
    const size_t cnt = (size_t)m * k + 1;
    if (tc->d_sidx.ensure(tc, cnt) != ICPMI_OK || tc->d_d2.ensure(tc, cnt) != ICPMI_OK) { c->last_error = tc->last_error; return ICPMI_ERR_HIP; }
    if (c->d_map_gi.ensure(c, (size_t)m + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    float* d_i = scratch_get<float>(c, 6, (size_t)m);
    float* d_is = scratch_get<float>(c, 7, (size_t)m);
    if (!d_i || !d_is) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(d_i, intensity, (size_t)m * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (tc->stream != c->stream) HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->dk_m = 0; // (as in ops_intensity_gradient)
    s = selfgrid_knn(tc, (const float4*)c->d_map_sorted, m, k, tc->d_sidx, tc->d_d2);
    if (s != ICPMI_OK) { c->last_error = tc->last_error; return s; }
    launch_intensity_gradient(tc, m, k, reinterpret_cast<const float*>(c->d_normals_sorted.get()), 4, d_i, (const float4*)c->d_map_sorted, d_is, nullptr,
                              c->d_map_gi);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(tc->stream)); // the caller's row is free on return
    c->gi_m = m; c->gi_version = c->map_version;
    return ICPMI_OK;
}

// Test seam (icpmi_debug_self_knn): the search of ops_surface_normals and nothing behind it -- the same private handle (its grid's tuning
// history is the filter's), ids through keepMatchedIds' conversion, d2 as the search kernels left them
icpmi_status ops_debug_self_knn(icpmi_ctx* c, const float* pts4, int64_t m, int k, int32_t* ids, float* d2, uint64_t* info)
{
    if (k < 1 || k > ICPMI_MAX_K) { c->last_error = "debug_self_knn: k must be in [1, 32]"; return ICPMI_ERR_INVALID_ARG; }
    TempCtx t;
    icpmi_status s = make_temp(c, t);
    if (s != ICPMI_OK) return s;
    s = temp_knn(c, t, pts4, m, nullptr, m, k, 1, true);
    if (s != ICPMI_OK) return s;
    icpmi_ctx* tc = t.h;
    const size_t cnt = (size_t)m * k;
    DevBuf<int> d_ids;
    HIP_TRY(c, d_ids.alloc(cnt));
    if (nn_ids_to_original(tc, tc->d_sidx, (int64_t)cnt, d_ids) != ICPMI_OK) { c->last_error = tc->last_error; return ICPMI_ERR_HIP; }
    HIP_TRY(c, hipMemcpyAsync(ids, d_ids, cnt * sizeof(int), hipMemcpyDeviceToHost, tc->stream));
    HIP_TRY(c, hipMemcpyAsync(d2, tc->d_d2, cnt * sizeof(float), hipMemcpyDeviceToHost, tc->stream));
    HIP_TRY(c, hipStreamSynchronize(tc->stream));
    if (info) {
        s = selfgrid_debug_info(tc, info);
        if (s != ICPMI_OK) c->last_error = tc->last_error;
    }
    return s;
}

icpmi_status ops_point_distance_keep(icpmi_ctx* c, const float* map4, int64_t m, const float* in4, int64_t n, float min_dist,
                                     uint8_t* keep)
{
    if (n == 0) return ICPMI_OK;
    if (m == 0) { memset(keep, 1, (size_t)n); return ICPMI_OK; } // no neighbour: d2 = +inf >= lim
    TempCtx t;
    icpmi_status s = make_temp(c, t);
    if (s != ICPMI_OK) return s;
    s = temp_knn(c, t, map4, m, in4, n, 1, 0, false);
    if (s != ICPMI_OK) return s;
    icpmi_ctx* tc = t.h;
    DevBuf<uint8_t> d_keep;
    HIP_TRY(c, d_keep.alloc((size_t)n));
    const double lim = pd_limit(min_dist);
    hipLaunchKernelGGL(keep_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, tc->stream, tc->d_d2, n, lim, d_keep);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, tc->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(tc->stream);
    HIP_TRY(c, e);
    return ICPMI_OK;
}

// decimation flags of a DEVICE cloud (T = uint8_t or unsigned), stream-ordered on c->stream
template <typename T>
icpmi_status voxel_flags_dev(icpmi_ctx* c, const float4* d_in, int64_t n, float edge, int method, T* d_keep)
{
    if (n > 0xfffffff0ll) { c->last_error = "voxel_keep: too many points"; return ICPMI_ERR_UNSUPPORTED; }
    unsigned long long cap = 1024;
    while (cap < (unsigned long long)n * 2ull) cap <<= 1;
    unsigned long long* d_keys = scratch_get<unsigned long long>(c, 0, (size_t)cap);
    unsigned* d_vals = scratch_get<unsigned>(c, 1, (size_t)cap);
    unsigned* d_slot = scratch_get<unsigned>(c, 2, (size_t)n);
    unsigned* d_lo = scratch_get<unsigned>(c, 3, 4);
    if (!d_keys || !d_vals || !d_slot || !d_lo) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemsetAsync(d_keys, 0xff, (size_t)cap * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(d_vals, 0xff, (size_t)cap * sizeof(unsigned), c->stream));
    HIP_TRY(c, hipMemsetAsync(d_lo, 0xff, 4 * sizeof(unsigned), c->stream));
    const int blocks = (int)((n + 255) / 256);
    const int rb = blocks < 1024 ? blocks : 1024;
    hipLaunchKernelGGL(bbox_min_kernel, dim3(rb), dim3(256), 0, c->stream, d_in, n, d_lo);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3(blocks), dim3(256), 0, c->stream, d_in, n, d_lo, edge, method, d_keys, d_vals, cap - 1, d_slot);
    hipLaunchKernelGGL(voxel_keep_kernel<T>, dim3(blocks), dim3(256), 0, c->stream, n, d_vals, d_slot, method, d_keep);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}
template icpmi_status voxel_flags_dev<uint8_t>(icpmi_ctx*, const float4*, int64_t, float, int, uint8_t*);
template icpmi_status voxel_flags_dev<unsigned>(icpmi_ctx*, const float4*, int64_t, float, int, unsigned*);

icpmi_status ops_filter_points(icpmi_ctx* c, const float* in4, int64_t n, const icpmi_point_filter* filters, int n_filters, uint8_t* keep)
{
    if (n == 0) return ICPMI_OK;
    FilterPack fp;
    fp.n = n_filters;
    for (int k = 0; k < n_filters; ++k) fp.f[k] = filters[k];
    if (c->d_stage_in.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    uint8_t* d_keep = scratch_get<uint8_t>(c, 9, (size_t)n);
    if (!d_keep) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(c->d_stage_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(filter_points_kernel, dim3((int)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_stage_in, n, fp, d_keep);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ICPMI_OK;
}

// the arguments are validated by icpmi_sensor_model (api.hip): every pointer the program needs is there, an output it does not produce is NULL
icpmi_status ops_sensor_model(icpmi_ctx* c, const float* in4, int64_t n, const float* normals3_in, const float* obs_dir3_in, const icpmi_sensor_step* steps,
                              int n_steps, float* normals3_out, float* obs_dir3_out, float* noise_out, uint8_t* keep_out)
{
    if (n == 0) return ICPMI_OK;
    SensorPack sp{};
    sp.n = n_steps;
    for (int k = 0; k < n_steps; ++k) sp.s[k] = steps[k];
    sp.read_n = normals3_in ? 1 : 0; sp.write_n = normals3_out ? 1 : 0;
    sp.read_od = obs_dir3_in ? 1 : 0; sp.write_od = obs_dir3_out ? 1 : 0;
    if (c->d_stage_in.ensure(c, (size_t)n + 1) != ICPMI_OK) return ICPMI_ERR_HIP;
    float* d_n3 = nullptr; float* d_od3 = nullptr; float* d_noise = nullptr; uint8_t* d_keep = nullptr;
    if (sp.read_n || sp.write_n) { if (c->d_stage_n3.ensure(c, (size_t)n * 3) != ICPMI_OK) return ICPMI_ERR_HIP; d_n3 = c->d_stage_n3; }
    if ((sp.read_od || sp.write_od) && !(d_od3 = scratch_get<float>(c, 6, (size_t)n * 3))) return ICPMI_ERR_HIP;
    if (noise_out && !(d_noise = scratch_get<float>(c, 7, (size_t)n))) return ICPMI_ERR_HIP;
    if (keep_out && !(d_keep = scratch_get<uint8_t>(c, 9, (size_t)n))) return ICPMI_ERR_HIP;
    HIP_TRY(c, hipMemcpyAsync(c->d_stage_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (sp.read_n) HIP_TRY(c, hipMemcpyAsync(d_n3, normals3_in, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (sp.read_od) HIP_TRY(c, hipMemcpyAsync(d_od3, obs_dir3_in, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(sensor_model_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->d_stage_in, n, sp, d_n3, d_od3, d_noise, d_keep);
    HIP_TRY(c, hipGetLastError());
    if (sp.write_n) HIP_TRY(c, hipMemcpyAsync(normals3_out, d_n3, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (sp.write_od) HIP_TRY(c, hipMemcpyAsync(obs_dir3_out, d_od3, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (noise_out) HIP_TRY(c, hipMemcpyAsync(noise_out, d_noise, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (keep_out) HIP_TRY(c, hipMemcpyAsync(keep_out, d_keep, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ICPMI_OK;
}

icpmi_status ops_voxel_keep_first(icpmi_ctx* c, const float* in4, int64_t n, float edge, int method, uint8_t* keep)
{
    if (n == 0) return ICPMI_OK;
    DevBuf<float4> d_in; DevBuf<uint8_t> d_keep;
    HIP_TRY(c, d_in.alloc((size_t)n));
    HIP_TRY(c, d_keep.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(d_in, in4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    icpmi_status s = voxel_flags_dev<uint8_t>(c, d_in, n, edge, method, d_keep);
    if (s != ICPMI_OK) return s;
    HIP_TRY(c, hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return ICPMI_OK;
}
