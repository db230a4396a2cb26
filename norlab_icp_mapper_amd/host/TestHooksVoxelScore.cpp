// TestHooksVoxelScore.cpp -- C entry points for the tests of the voxel pose score in the host shell (tests/host_voxel_score_bindings.py):
// nim::rankVoxelCandidates (no GPU), GpuICPSequence::voxelScores / relocalizeVoxel and Mapper::relocalizeVoxel.
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
} // namespace

extern "C" {

// nim::rankVoxelCandidates over a hand-written table; order_out has room for n_cand indices.  Returns how many survive.
int nim_test_rank_voxel_candidates(const int32_t* status, const int64_t* pairs, const double* likelihood, int n_cand, int64_t n, float min_pairs_ratio,
                                   int32_t* order_out)
{
    nim::VoxelPoseScores sc;
    sc.score.assign((size_t)n_cand, icpmi_voxel_score{});
    sc.status.assign((size_t)n_cand, ICPMI_OK);
    for (int i = 0; i < n_cand; ++i) {
        sc.status[(size_t)i] = (icpmi_status)status[i];
        sc.score[(size_t)i].pairs = pairs[i];
        sc.score[(size_t)i].likelihood = likelihood[i];
    }
    const std::vector<int> order = nim::rankVoxelCandidates(sc, (size_t)n, min_pairs_ratio);
    for (size_t i = 0; i < order.size(); ++i) order_out[i] = order[i];
    return (int)order.size();
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap(map4 + map_normals3), then -- refine < 0 -- voxelScores(scan, candidates,
// level, beta) alone (scores_out / status_out), or relocalizeVoxel(scan, candidates, {refine, level, beta, min_pairs_ratio}): the winner's
// pose, score and index, and every candidate's first score.  Returns 0; 2 ConvergenceError, 1 any other exception, the text in err.
int nim_test_icp_relocalize_voxel(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                                  const float* scan_normals3, const float* cand16, int n_cand, int refine, int level, float beta,
                                  float min_pairs_ratio, float* pose_out16, icpmi_voxel_score* score_out, int32_t* index_out,
                                  icpmi_voxel_score* scores_out, int32_t* status_out, char* err, int err_cap)
{
    try {
        const nim::DataPoints map = cloud(map4, m, map_normals3), scan = cloud(scan4, n, scan_normals3);
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(map)) throw std::runtime_error("setMap refused the map");
        const std::vector<nim::Mat4> cand = mats(cand16, n_cand);
        nim::VoxelPoseScores first;
        if (refine < 0) first = icp.voxelScores(scan, cand, level, beta);
        else {
            nim::RelocalizeVoxelOptions opt;
            opt.refine = refine; opt.level = level; opt.beta = beta; opt.minPairsRatio = min_pairs_ratio;
            const nim::VoxelRelocalization r = icp.relocalizeVoxel(scan, cand, opt);
            std::memcpy(pose_out16, r.pose.data(), sizeof(float) * 16);
            *score_out = r.score;
            *index_out = r.index;
            first = r.scores;
        }
        for (int i = 0; i < n_cand; ++i) { scores_out[i] = first.score[(size_t)i]; status_out[i] = (int32_t)first.status[(size_t)i]; }
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2, err, err_cap);
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

// Mapper (offline, mapping on) from the configuration file `config`: setMap(map4 + map_normals3), relocalizeVoxel(scan, candidates, stamp 0).
// Out: the pose the call returned, getPose() afterwards, the winner's index and the map's size before and after the call.
int nim_test_mapper_relocalize_voxel(const char* config, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                                     const float* scan_normals3, const float* cand16, int n_cand, float* pose_out16, float* get_pose16,
                                     int32_t* index_out, int64_t* map_before, int64_t* map_after, char* err, int err_cap)
{
    try {
        const nim::DataPoints map = cloud(map4, m, map_normals3), scan = cloud(scan4, n, scan_normals3);
        nim::Mapper mapper(config, true, false, true, false);
        mapper.setMap(map);
        *map_before = (int64_t)mapper.getMap().getNbPoints();
        const nim::VoxelRelocalization r = mapper.relocalizeVoxel(scan, mats(cand16, n_cand), nim::TimePoint{std::chrono::nanoseconds(0)});
        std::memcpy(pose_out16, r.pose.data(), sizeof(float) * 16);
        std::memcpy(get_pose16, mapper.getPose().data(), sizeof(float) * 16);
        *index_out = r.index;
        *map_after = (int64_t)mapper.getMap().getNbPoints();
        return 0;
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

} // extern "C"
