// TestHooks.cpp -- a C entry into the host shell for the Python parity tests (tests/test_host_filters.py): runs a YAML sequence
// of DataPointsFilters (what `input:` / `post:` / the ICP chains' filter lists hold) on one cloud.  Not part of the reference
// surface; the product never calls it.
#include <cstring>

#include "IcpSequence.h"
#include "Mapper.h"

namespace nim { uint32_t minstdNth(uint32_t seed, uint32_t n); } // DataPointsFilters.cpp: the generator RandomSampling / MaxDensity / SamplingSurfaceNormal draw from

// the one body of nim_test_filter_chain and nim_test_filter_chain_times: every input and output beyond in4 / out4 / n_out may be NULL
static int filterChain(icpmi_handle h, const char* yaml_seq, const float* in4, int64_t n, const char* desc_name, int desc_span, const float* desc,
                       const char* time_name, int time_span, const int64_t* times, float* out4, float* out_normals3, float* out_desc,
                       int64_t* out_times, int64_t* n_out, int* has_normals, char* err, int err_cap)
{
    try {
        nim::DataPoints c((size_t)n);
        std::memcpy(c.features.data(), in4, sizeof(float) * 4 * (size_t)n);
        if (desc_name && desc) c.addDescriptor(desc_name, desc_span, std::vector<float>(desc, desc + (size_t)desc_span * n));
        if (time_name && times) c.addTime(time_name, time_span, std::vector<int64_t>(times, times + (size_t)time_span * n));
        nim::DataPointsFilters chain(nim::yaml::Load(yaml_seq), h);
        chain.apply(c);
        const size_t m = c.getNbPoints();
        std::memcpy(out4, c.features.data(), sizeof(float) * 4 * m);
        const bool hn = c.descriptorExists("normals");
        if (has_normals) *has_normals = hn ? 1 : 0;
        if (hn && out_normals3) std::memcpy(out_normals3, c.getDescriptorByName("normals").data.data(), sizeof(float) * 3 * m);
        if (desc_name && out_desc && c.descriptorExists(desc_name)) std::memcpy(out_desc, c.getDescriptorByName(desc_name).data.data(), sizeof(float) * (size_t)desc_span * m);
        if (time_name && out_times && c.timeExists(time_name)) {
            const std::vector<int64_t>& t = c.getTimeByName(time_name).data;
            if (t.size() != (size_t)time_span * m) throw std::logic_error("the filter chain left `times` out of step with the points");
            std::memcpy(out_times, t.data(), sizeof(int64_t) * t.size());
        }
        *n_out = (int64_t)m;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

extern "C" {

// the raw n-th value of the host filters' std::minstd_rand restatement ([rand.predef]: seed 1, n = 10 000 -> 399268537)
uint32_t nim_test_minstd_nth(uint32_t seed, uint32_t n) { return nim::minstdNth(seed, n); }

// yaml_seq: e.g. "- RandomSamplingDataPointsFilter: {prob: 0.5, seed: 3}".  in: 4 x n features + optional descriptor `desc_name`
// (span x n).  out4 (capacity 4 n), out_normals3 (3 n, may be NULL: receives `normals` if the result has them), out_desc (span x n,
// may be NULL: the input descriptor after filtering).  Returns 0, or 1 with the exception text in err.
int nim_test_filter_chain(icpmi_handle h, const char* yaml_seq, const float* in4, int64_t n, const char* desc_name, int desc_span,
                          const float* desc, float* out4, float* out_normals3, float* out_desc, int64_t* n_out, int* has_normals,
                          char* err, int err_cap)
{
    return filterChain(h, yaml_seq, in4, n, desc_name, desc_span, desc, nullptr, 0, nullptr, out4, out_normals3, out_desc, nullptr, n_out, has_normals, err, err_cap);
}

// the same with one float descriptor AND one int64 `times` row group (`time_name`, time_span x n, may be NULL): out_times
// (time_span x n) receives it after filtering.  Descriptors and times are (span x n) column-major, like the DataPoints.
int nim_test_filter_chain_times(icpmi_handle h, const char* yaml_seq, const float* in4, int64_t n, const char* desc_name, int desc_span,
                                const float* desc, const char* time_name, int time_span, const int64_t* times, float* out4, float* out_desc,
                                int64_t* out_times, int64_t* n_out, char* err, int err_cap)
{
    return filterChain(h, yaml_seq, in4, n, desc_name, desc_span, desc, time_name, time_span, times, out4, nullptr, out_desc, out_times, n_out, nullptr, err, err_cap);
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp) (the `icp:` sub-tree), setMap(in4), then the resident map as the core holds it
// (downloadMap): what the referenceDataPointsFilters chain made of the cloud.  out4: capacity 4 n.  Returns 0, or 1 with the text in err.
int nim_test_icp_set_map(const char* yaml_icp, const float* in4, int64_t n, float* out4, int64_t* n_out, char* err, int err_cap)
{
    try {
        nim::DataPoints c((size_t)n);
        std::memcpy(c.features.data(), in4, sizeof(float) * 4 * (size_t)n);
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        *n_out = 0;
        if (!icp.setMap(c)) return 0;
        const nim::DataPoints m = icp.downloadMap();
        if (m.getNbPoints() > (size_t)n) throw std::runtime_error("the resident map is larger than the input");
        std::memcpy(out4, m.features.data(), sizeof(float) * 4 * m.getNbPoints());
        *n_out = (int64_t)m.getNbPoints();
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// The offline replay of build_map_from_scans_and_trajectory (Mapper on device 0, 3-D, mapping) over the scan files `paths` with the given
// poses (column-major 4 x 4 each) and stamps; after every processInput the mapper's pose goes to poses_out16 and, when the ICP chain has
// PointToPlaneWithCovErrorMinimizer and that scan was registered, errorMinimizer->getCovariance() to cov36 (cov_ok[i] = 1; else 0).
int nim_test_mapper_replay(const char* config, int n_scans, const char* const* paths, const float* poses16, const int64_t* stamps_ns,
                           float* poses_out16, float* cov36, int32_t* cov_ok, char* err, int err_cap)
{
    try {
        nim::Mapper mapper(config, true, false, true, false);
        for (int i = 0; i < n_scans; ++i) {
            nim::DataPoints cloud = nim::DataPoints::load(paths[i]);
            mapper.applyInputFilters(cloud);
            nim::Mat4 pose;
            std::memcpy(pose.data(), poses16 + 16 * i, sizeof(float) * 16);
            mapper.processInput(cloud, pose, nim::TimePoint{std::chrono::nanoseconds(stamps_ns[i])});
            std::memcpy(poses_out16 + 16 * i, mapper.getPose().data(), sizeof(float) * 16);
            cov_ok[i] = 0;
            try {
                const std::array<float, 36> c = mapper.icpSequence().errorMinimizer->getCovariance();
                std::memcpy(cov36 + 36 * i, c.data(), sizeof c);
                cov_ok[i] = 1;
            } catch (const std::exception&) {}
        }
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

} // extern "C"
