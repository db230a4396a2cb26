// TestHooksGlobalLocalize.cpp -- C entry points for the tests of the global localisation in the host shell
// (tests/host_global_localize_bindings.py): nim::yawRotations (no GPU), GpuICPSequence::globalLocalize / relocalizeGlobal and
// Mapper::relocalizeGlobal.
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "IcpSequence.h"
#include "Mapper.h"

namespace {
int fail(const std::exception& e, int rc, char* err, int err_cap)
{
    if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return rc;
}

nim::DataPoints cloud(const float* pts4, int64_t n, const float* normals3)
{
    nim::DataPoints c((size_t)n);
    std::memcpy(c.features.data(), pts4, sizeof(float) * 4 * (size_t)n);
    if (normals3) c.addDescriptor("normals", 3, std::vector<float>(normals3, normals3 + 3 * (size_t)n));
    return c;
}

std::vector<nim::Rot9> rots(const float* r9, int count)
{
    std::vector<nim::Rot9> out((size_t)count);
    for (int i = 0; i < count; ++i) std::memcpy(out[(size_t)i].data(), r9 + 9 * i, sizeof(float) * 9);
    return out;
}

nim::GlobalLocalizeOptions options(float cell, int levels, float ratio, int64_t max_nodes, int batch, const double* box6)
{
    nim::GlobalLocalizeOptions o;
    o.cellSize = cell; o.levels = levels; o.minScoreRatio = ratio; o.maxNodes = max_nodes; o.batch = batch;
    if (box6) {
        o.hasBox = true;
        for (int j = 0; j < 3; ++j) { o.boxLo[(size_t)j] = box6[j]; o.boxHi[(size_t)j] = box6[3 + j]; }
    }
    return o;
}
} // namespace

extern "C" {

// nim::yawRotations: out9 has room for steps blocks of 9 floats (column-major).  Returns 0; 1 on an exception.
int nim_test_yaw_rotations(int steps, double roll, double pitch, float* out9, char* err, int err_cap)
{
    try {
        const std::vector<nim::Rot9> r = nim::yawRotations(steps, roll, pitch);
        for (size_t i = 0; i < r.size(); ++i) std::memcpy(out9 + 9 * i, r[i].data(), sizeof(float) * 9);
        return 0;
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap(map4 + map_normals3), then globalLocalize (refine == 0: result_out alone) or
// relocalizeGlobal, whose refinement takes one candidate with refine = 1: result_out, the refined pose, and the refinement's residual or
// voxel score (whichever the chain has; the other stays zero).  box6: lo then hi, or null.  Returns 0; 2 ConvergenceError, 1 otherwise.
int nim_test_icp_global_localize(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                                 const float* scan_normals3, const float* r9, int n_rot, float cell, int levels, float ratio, int64_t max_nodes,
                                 int batch, const double* box6, int refine, icpmi_global_localize_result* result_out, float* pose_out16,
                                 icpmi_residual* residual_out, icpmi_voxel_score* score_out, int32_t* voxel_out, char* err, int err_cap)
{
    try {
        const nim::DataPoints map = cloud(map4, m, map_normals3), scan = cloud(scan4, n, scan_normals3);
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(map)) throw std::runtime_error("setMap refused the map");
        const nim::GlobalLocalizeOptions o = options(cell, levels, ratio, max_nodes, batch, box6);
        if (!refine) { *result_out = icp.globalLocalize(scan, rots(r9, n_rot), o); return 0; }
        nim::RelocalizeOptions ro; ro.refine = 1;
        nim::RelocalizeVoxelOptions vo; vo.refine = 1;
        const nim::GlobalRelocalization g = icp.relocalizeGlobal(scan, rots(r9, n_rot), o, ro, vo);
        *result_out = g.search;
        std::memcpy(pose_out16, g.pose.data(), sizeof(float) * 16);
        *residual_out = g.refined.residual;
        *score_out = g.refinedVoxel.score;
        *voxel_out = g.voxel ? 1 : 0;
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2, err, err_cap);
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

// Mapper (offline, mapping on) from the configuration file `config`: setMap(map4 + map_normals3), relocalizeGlobal(scan, rotations, stamp 0)
// with refine = 1.  Out: the search's result, the pose the call returned, getPose() afterwards and the map's size before and after.
int nim_test_mapper_relocalize_global(const char* config, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                                      const float* scan_normals3, const float* r9, int n_rot, float cell, int levels, const double* box6,
                                      icpmi_global_localize_result* result_out, float* pose_out16, float* get_pose16, int64_t* map_before,
                                      int64_t* map_after, char* err, int err_cap)
{
    try {
        const nim::DataPoints map = cloud(map4, m, map_normals3), scan = cloud(scan4, n, scan_normals3);
        nim::Mapper mapper(config, true, false, true, false);
        mapper.setMap(map);
        *map_before = (int64_t)mapper.getMap().getNbPoints();
        nim::RelocalizeOptions ro; ro.refine = 1;
        nim::RelocalizeVoxelOptions vo; vo.refine = 1;
        const nim::GlobalRelocalization g = mapper.relocalizeGlobal(scan, rots(r9, n_rot), nim::TimePoint{std::chrono::nanoseconds(0)},
                                                                    options(cell, levels, 0.f, 0, 64, box6), ro, vo);
        *result_out = g.search;
        std::memcpy(pose_out16, g.pose.data(), sizeof(float) * 16);
        std::memcpy(get_pose16, mapper.getPose().data(), sizeof(float) * 16);
        *map_after = (int64_t)mapper.getMap().getNbPoints();
        return 0;
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

} // extern "C"
