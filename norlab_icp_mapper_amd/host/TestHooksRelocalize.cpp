// TestHooksRelocalize.cpp -- C entry points for the tests of the relocalisation calls (tests/relocalize_bindings.py): the ranking and the
// candidate grid (no GPU), GpuICPSequence::relocalize and Mapper::relocalize.
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
} // namespace

extern "C" {

// nim::rankCandidates over a hand-written table; order_out has room for n_cand indices.  Returns how many survive.
int nim_test_rank_candidates(const int32_t* status, const int64_t* pairs, const double* sum_abs, int n_cand, int64_t n, float min_pairs_ratio,
                             int32_t* order_out)
{
    nim::PoseScores sc;
    sc.residual.assign((size_t)n_cand, icpmi_residual{});
    sc.status.assign((size_t)n_cand, ICPMI_OK);
    for (int i = 0; i < n_cand; ++i) {
        sc.status[(size_t)i] = (icpmi_status)status[i];
        sc.residual[(size_t)i].pairs = pairs[i];
        sc.residual[(size_t)i].sum_abs = sum_abs[i];
    }
    const std::vector<int> order = nim::rankCandidates(sc, (size_t)n, min_pairs_ratio);
    for (size_t i = 0; i < order.size(); ++i) order_out[i] = order[i];
    return (int)order.size();
}

// nim::candidateGrid; out16 has room for cap poses (column-major).  Returns the number of poses, -1 when they do not fit or on an exception.
int nim_test_candidate_grid(const float* centre16, float half_x, float half_y, float half_yaw, int steps_x, int steps_y, int steps_yaw,
                            float* out16, int cap)
{
    try {
        nim::Mat4 c;
        std::memcpy(c.data(), centre16, sizeof(float) * 16);
        const std::vector<nim::Mat4> g = nim::candidateGrid(c, half_x, half_y, half_yaw, steps_x, steps_y, steps_yaw);
        if ((int)g.size() > cap) return -1;
        for (size_t i = 0; i < g.size(); ++i) std::memcpy(out16 + 16 * i, g[i].data(), sizeof(float) * 16);
        return (int)g.size();
    } catch (const std::exception&) {
        return -1;
    }
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap(map4 + map_normals3), relocalize(scan4, candidates).  Out: the winner's
// pose, residual and index, the score table (n_cand residuals and statuses, batched), and -- ms_T16 != NULL -- the corrections and
// statuses of registerMultiStart(scan, {candidates[ms_index]}) called alone afterwards.  Returns 0; 2 ConvergenceError, 3 InvalidField,
// 4 InvalidParameter, 1 any other exception, the text in err.
int nim_test_icp_relocalize(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                            const float* cand16, int n_cand, float min_pairs_ratio, int refine, int kind, float* pose_out16,
                            icpmi_residual* res_out, int32_t* index_out, icpmi_residual* scores_out, int32_t* status_out, int32_t* batched_out,
                            int ms_index, float* ms_T16, int32_t* ms_status, char* err, int err_cap)
{
    try {
        nim::DataPoints map((size_t)m), scan((size_t)n);
        std::memcpy(map.features.data(), map4, sizeof(float) * 4 * (size_t)m);
        if (map_normals3) map.addDescriptor("normals", 3, std::vector<float>(map_normals3, map_normals3 + 3 * (size_t)m));
        std::memcpy(scan.features.data(), scan4, sizeof(float) * 4 * (size_t)n);
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(map)) throw std::runtime_error("setMap refused the map");
        const std::vector<nim::Mat4> cand = mats(cand16, n_cand);
        nim::RelocalizeOptions opt;
        opt.minPairsRatio = min_pairs_ratio; opt.refine = refine; opt.kind = kind;
        const nim::Relocalization r = icp.relocalize(scan, cand, opt);
        std::memcpy(pose_out16, r.pose.data(), sizeof(float) * 16);
        *res_out = r.residual;
        *index_out = r.index;
        for (int i = 0; i < n_cand; ++i) { scores_out[i] = r.scores.residual[(size_t)i]; status_out[i] = (int32_t)r.scores.status[(size_t)i]; }
        *batched_out = r.scores.batched;
        if (ms_T16) {
            const nim::MultiStartResult ms = icp.registerMultiStart(scan, {cand[(size_t)ms_index]});
            std::memcpy(ms_T16, ms.correction[0].data(), sizeof(float) * 16);
            *ms_status = (int32_t)ms.status[0];
        }
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2, err, err_cap);
    } catch (const nim::InvalidField& e) {
        return fail(e, 3, err, err_cap);
    } catch (const nim::InvalidParameter& e) {
        return fail(e, 4, err, err_cap);
    } catch (const std::exception& e) {
        return fail(e, 1, err, err_cap);
    }
}

// Mapper (offline, mapping on) from the configuration file `config`: setMap(map4 + map_normals3), relocalize(scan4, candidates, stamp 0).
// Out: the pose relocalize returned, getPose() afterwards, the winner's index and the map's size before and after the call.
int nim_test_mapper_relocalize(const char* config, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                               const float* cand16, int n_cand, float* pose_out16, float* get_pose16, int32_t* index_out, int64_t* map_before,
                               int64_t* map_after, char* err, int err_cap)
{
    try {
        nim::DataPoints map((size_t)m), scan((size_t)n);
        std::memcpy(map.features.data(), map4, sizeof(float) * 4 * (size_t)m);
        if (map_normals3) map.addDescriptor("normals", 3, std::vector<float>(map_normals3, map_normals3 + 3 * (size_t)m));
        std::memcpy(scan.features.data(), scan4, sizeof(float) * 4 * (size_t)n);
        nim::Mapper mapper(config, true, false, true, false);
        mapper.setMap(map);
        *map_before = (int64_t)mapper.getMap().getNbPoints();
        const nim::Relocalization r = mapper.relocalize(scan, mats(cand16, n_cand), nim::TimePoint{std::chrono::nanoseconds(0)});
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
