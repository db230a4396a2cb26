// maxdensity.hip -- MaxDensityDataPointsFilter's draw on the device (include/icpmi.h: icpmi_max_density_keep; the host filter it restates:
// host/DataPointsFilters.cpp, MaxDensityFilter).  The host filter walks the cloud with ONE std::minstd_rand and takes a number for every
// dense point only: point i reads the (rank_i + 1)-th number of the stream, rank_i = how many dense points stand in front of it.  Here the
// rank is an exclusive prefix count of the dense flags (the handle's scan, map_build.hip) and the number comes from the skip-ahead
// (common.h: minstd_nth, as in ssn.hip / normalspace.hip): every point decides on its own, no atomics, two calls give the same bits.
#include "common.h"

namespace {

// dense[i] = densities[i] > max_density (a NaN density compares false: not dense)
__global__ __launch_bounds__(256) void maxdens_dense_kernel(int64_t n, const float* __restrict__ dens, float max_density, unsigned* __restrict__ dense)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dense[i] = dens[i] > max_density ? 1u : 0u;
}

// keep[i] = dense ? u < max_density / density : 1, u = (float)x / 2147483645.0f with x the (rank[i] + 1)-th number of the stream: float32
// throughout, both divisions correctly rounded (the build's default for HIP; -ffp-contract=off: nothing is fused), as the host's
// `rng.unit(0) < maxDensity / density`.  A +inf density gives the bound 0 and is dropped (u < 0 is false).
template <class T>
__global__ __launch_bounds__(256) void maxdens_draw_kernel(int64_t n, const float* __restrict__ dens, const unsigned* __restrict__ rank, float max_density,
                                                           unsigned seed, T* __restrict__ keep)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float d = dens[i];
    T k = 1;
    if (d > max_density) {
        const unsigned x = minstd_nth(seed, rank[i] + 1u);
        k = ((float)x / 2147483645.0f) < (max_density / d) ? 1 : 0;
    }
    keep[i] = k;
}

// d_work / d_rank: n + 1 words each (the scan writes its total behind the ranks)
template <class T>
icpmi_status max_density_draw(icpmi_ctx* c, const float* d_dens, int64_t n, float max_density, int seed, unsigned* d_work, unsigned* d_rank, T* d_keep)
{
    const int blocks = (int)((n + 255) / 256);
    hipLaunchKernelGGL(maxdens_dense_kernel, dim3(blocks), dim3(256), 0, c->stream, n, d_dens, max_density, d_work);
    const icpmi_status s = device_exclusive_scan_io(c, d_work, d_rank, (int)n, 0u);
    if (s != ICPMI_OK) return s;
    hipLaunchKernelGGL(maxdens_draw_kernel<T>, dim3(blocks), dim3(256), 0, c->stream, n, d_dens, (const unsigned*)d_rank, max_density, (unsigned)seed, d_keep);
    HIP_TRY(c, hipGetLastError());
    return ICPMI_OK;
}

} // namespace

bool max_density_param_ok(float max_density) { return std::isfinite(max_density) && max_density > 0.f; }

// the map-update chain's step: the 0 / 1 keep flags of the working map's density row into d_flag; d_rank is scratch (n + 1 words each)
icpmi_status max_density_flags_dev(icpmi_ctx* c, const float* d_dens, int64_t n, float max_density, int seed, unsigned* d_flag, unsigned* d_rank)
{
    if (n == 0) return ICPMI_OK;
    return max_density_draw(c, d_dens, n, max_density, seed, d_flag, d_rank, d_flag); // (the draw reads the densities again, not the dense flags it overwrites)
}

icpmi_status ops_max_density_keep(icpmi_ctx* c, const float* densities, int64_t n, float max_density, int seed, uint8_t* keep)
{
    if (n == 0) return ICPMI_OK;
    DevBuf<float> d_dens; DevBuf<unsigned> d_work, d_rank; DevBuf<uint8_t> d_keep;
    HIP_TRY(c, d_dens.alloc((size_t)n)); HIP_TRY(c, d_work.alloc((size_t)n + 1)); HIP_TRY(c, d_rank.alloc((size_t)n + 1)); HIP_TRY(c, d_keep.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(d_dens.get(), densities, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    const icpmi_status s = max_density_draw(c, d_dens.get(), n, max_density, seed, d_work.get(), d_rank.get(), d_keep.get());
    if (s != ICPMI_OK) return s;
    HIP_TRY(c, hipMemcpyAsync(keep, d_keep.get(), (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream)); // the scratch of this call is freed on return
    return ICPMI_OK;
}
