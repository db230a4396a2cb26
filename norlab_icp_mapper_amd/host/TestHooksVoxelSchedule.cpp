// TestHooksVoxelSchedule.cpp -- C entry points for the tests of VoxelMatcher's voxelSizes in the host shell (tests/test_voxel_pyramid_cpu.py,
// tests/test_gpu_voxel_pyramid.py): the YAML key as parseMatcher reads it, and one GpuICPSequence registration with its per-level report.
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "IcpSequence.h"

namespace {
int fail(const std::exception& e, char* err, int err_cap)
{
    if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return 1;
}
} // namespace

extern "C" {

// parseMatcher on the `matcher:` entry given as YAML text (no GPU, no handle): the schedule (*n_sizes entries of sizes4, 0 when the entry has
// no voxelSizes) and the voxel size (the finest of them).  Returns 0, or 1 with the exception's text in err.
int nim_test_parse_voxel_schedule(const char* yaml_matcher, float* voxel_size, float sizes4[4], int* n_sizes, char* err, int err_cap)
{
    try {
        icpmi_config cfg;
        icpmi_config_default(&cfg);
        std::string field;
        std::vector<float> sizes;
        nim::parseMatcher(nim::yaml::Load(yaml_matcher), cfg, field, voxel_size, &sizes);
        *n_sizes = (int)sizes.size();
        for (size_t i = 0; i < sizes.size() && i < 4; ++i) sizes4[i] = sizes[i];
        return 0;
    } catch (const std::exception& e) { return fail(e, err, err_cap); }
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap(map4 + map_normals3), operator() on the reading (scan4 + scan_normals3 as
// `normals`), then voxelScheduleReport(): *levels entries of iterations4 / pairs_first4 / pairs_last4.  T_out16 column-major.
int nim_test_icp_register_voxel_schedule(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                                         const float* scan_normals3, float* T_out16, icpmi_stats* stats_out, int* levels, int* iterations4,
                                         int* pairs_first4, int* pairs_last4, char* err, int err_cap)
{
    try {
        nim::DataPoints map((size_t)m), scan((size_t)n);
        std::memcpy(map.features.data(), map4, sizeof(float) * 4 * (size_t)m);
        map.addDescriptor("normals", 3, std::vector<float>(map_normals3, map_normals3 + 3 * (size_t)m));
        std::memcpy(scan.features.data(), scan4, sizeof(float) * 4 * (size_t)n);
        scan.addDescriptor("normals", 3, std::vector<float>(scan_normals3, scan_normals3 + 3 * (size_t)n));
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(map)) throw std::runtime_error("setMap refused the map");
        const nim::Mat4 T = icp(scan);
        std::memcpy(T_out16, T.data(), sizeof(float) * 16);
        *stats_out = icp.stats();
        const std::vector<nim::GpuICPSequence::VoxelLevelReport> rep = icp.voxelScheduleReport();
        *levels = (int)rep.size();
        for (size_t l = 0; l < rep.size() && l < 4; ++l) { iterations4[l] = rep[l].iterations; pairs_first4[l] = rep[l].pairsFirst; pairs_last4[l] = rep[l].pairsLast; }
        return 0;
    } catch (const std::exception& e) { return fail(e, err, err_cap); }
}

} // extern "C"
