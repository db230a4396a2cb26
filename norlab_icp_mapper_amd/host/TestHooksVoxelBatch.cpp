// TestHooksVoxelBatch.cpp -- C entry points for the tests of the voxel batch in the host shell (tests/voxel_batch_cases.py):
// GpuICPSequence::registerVoxelBatch / registerVoxelMultiStart and relocalizeVoxel with the handle's call counters around it.
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "IcpSequence.h"

namespace {
int fail(const std::exception& e, int rc, char* err, int err_cap)
{
    if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return rc;
}

std::vector<nim::Mat4> mats(const float* m16, int count)
{
    std::vector<nim::Mat4> out((size_t)count);
    for (int i = 0; i < count; ++i) std::memcpy(out[(size_t)i].data(), m16 + 16 * i, sizeof(float) * 16);
    return out;
}

nim::DataPoints cloud(const float* pts4, int64_t n, const float* normals3)
{
    nim::DataPoints c((size_t)n);
    std::memcpy(c.features.data(), pts4, sizeof(float) * 4 * (size_t)n);
    if (normals3) c.addDescriptor("normals", 3, std::vector<float>(normals3, normals3 + 3 * (size_t)n));
    return c;
}

void result_out(const nim::MultiStartResult& r, float* T_out16, int32_t* status_out, int32_t* iterations_out, int64_t* pairs_out)
{
    for (size_t i = 0; i < r.status.size(); ++i) {
        std::memcpy(T_out16 + 16 * i, r.correction[i].data(), sizeof(float) * 16);
        status_out[i] = (int32_t)r.status[i];
        iterations_out[i] = r.stats[i].iterations;
        pairs_out[i] = r.stats[i].pairs;
    }
}
} // namespace

extern "C" {

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap, then registerVoxelBatch over `batch` readings laid end to end in scans4 /
// scan_normals3 (counts[b] points each), or -- priors16 != NULL -- registerVoxelMultiStart(the first reading, n_priors priors).
// Out per member: the correction (column-major), its status, iterations and pairs; stats_iterations: stats().iterations afterwards.
// Returns 0; 1 any exception, the text in err.
int nim_test_icp_voxel_batch(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scans4, const float* scan_normals3,
                             const int64_t* counts, int batch, const float* priors16, int n_priors, float* T_out16, int32_t* status_out,
                             int32_t* iterations_out, int64_t* pairs_out, int32_t* stats_iterations, char* err, int err_cap)
{
    try {
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(cloud(map4, m, map_normals3))) throw std::runtime_error("setMap refused the map");
        std::vector<nim::DataPoints> readings;
        int64_t off = 0;
        for (int b = 0; b < batch; ++b) { readings.push_back(cloud(scans4 + 4 * off, counts[b], scan_normals3 + 3 * off)); off += counts[b]; }
        const nim::MultiStartResult r = priors16 ? icp.registerVoxelMultiStart(readings.at(0), mats(priors16, n_priors)) : icp.registerVoxelBatch(readings);
        result_out(r, T_out16, status_out, iterations_out, pairs_out);
        *stats_iterations = icp.stats().iterations;
        return 0;
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

// ... relocalizeVoxel(scan, candidates, {refine, level, beta}) with icpmi_debug_voxel_batch_calls read before and after it: calls_out[0..3) =
// loops of the voxel batch, members they carried and single registrations on the voxel path that the call made.
// Returns 0; 2 ConvergenceError, 1 any other exception.
int nim_test_icp_relocalize_voxel_counted(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                                          const float* scan_normals3, const float* cand16, int n_cand, int refine, int level, float beta,
                                          float* pose_out16, icpmi_voxel_score* score_out, int32_t* index_out, int64_t* calls_out,
                                          int32_t* stats_iterations, char* err, int err_cap)
{
    try {
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(cloud(map4, m, map_normals3))) throw std::runtime_error("setMap refused the map");
        nim::RelocalizeVoxelOptions opt;
        opt.refine = refine; opt.level = level; opt.beta = beta;
        int64_t before[3] = {0, 0, 0}, after[3] = {0, 0, 0};
        nim::GpuICPSequence::check(icp.handle(), icpmi_debug_voxel_batch_calls(icp.handle(), before));
        const nim::VoxelRelocalization r = icp.relocalizeVoxel(cloud(scan4, n, scan_normals3), mats(cand16, n_cand), opt);
        nim::GpuICPSequence::check(icp.handle(), icpmi_debug_voxel_batch_calls(icp.handle(), after));
        for (int i = 0; i < 3; ++i) calls_out[i] = after[i] - before[i];
        std::memcpy(pose_out16, r.pose.data(), sizeof(float) * 16);
        *score_out = r.score;
        *index_out = r.index;
        *stats_iterations = icp.stats().iterations;
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2, err, err_cap);
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

} // extern "C"
