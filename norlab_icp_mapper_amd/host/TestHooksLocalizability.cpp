// TestHooksLocalizability.cpp -- C entry points for the tests of the degeneracy-aware point-to-plane solve in the host shell
// (tests/test_gpu_localizability.py): the YAML keys of the minimiser and the Mapper replay with its report and its map-update veto.
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>

#include "IcpSequence.h"
#include "Mapper.h"

namespace {
int fail(const std::exception& e, char* err, int err_cap)
{
    if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return 1;
}
} // namespace

extern "C" {

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp) (the `icp:` sub-tree); *threshold_out = icpmi_config::degeneracy_threshold as parsed
int nim_test_icp_degeneracy_yaml(const char* yaml_icp, float* threshold_out, char* err, int err_cap)
{
    try {
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        *threshold_out = icp.config().degeneracy_threshold;
        return 0;
    } catch (const std::exception& e) { return fail(e, err, err_cap); }
}

// nim_test_mapper_replay with the degeneracy report instead of the covariance: after every processInput the mapper's pose goes to
// poses_out16, Mapper::getLocalizability() to loc[i] when there is one (loc_ok[i] = 1; else 0) and lastScanStartedMapUpdate() to grew[i].
// max_degenerate: Mapper::setMaxDegenerateDirectionsForUpdate.
int nim_test_mapper_replay_localizability(const char* config, int n_scans, const char* const* paths, const float* poses16, const int64_t* stamps_ns,
                                          int max_degenerate, float* poses_out16, icpmi_localizability* loc, int32_t* loc_ok, int32_t* grew,
                                          char* err, int err_cap)
{
    try {
        nim::Mapper mapper(config, true, false, true, false);
        mapper.setMaxDegenerateDirectionsForUpdate(max_degenerate);
        for (int i = 0; i < n_scans; ++i) {
            nim::DataPoints cloud = nim::DataPoints::load(paths[i]);
            mapper.applyInputFilters(cloud);
            nim::Mat4 pose;
            std::memcpy(pose.data(), poses16 + 16 * i, sizeof(float) * 16);
            mapper.processInput(cloud, pose, nim::TimePoint{std::chrono::nanoseconds(stamps_ns[i])});
            std::memcpy(poses_out16 + 16 * i, mapper.getPose().data(), sizeof(float) * 16);
            loc_ok[i] = mapper.lastLocalizabilityIsValid() ? 1 : 0;
            if (loc_ok[i]) loc[i] = mapper.getLocalizability();
            grew[i] = mapper.lastScanStartedMapUpdate() ? 1 : 0;
        }
        return 0;
    } catch (const std::exception& e) { return fail(e, err, err_cap); }
}

} // extern "C"
