// TestHooks.cpp -- a C entry into the host shell for the Python parity tests (tests/test_host_filters.py): runs a YAML sequence
// of DataPointsFilters (what `input:` / `post:` / the ICP chains' filter lists hold) on one cloud.  Not part of the reference
// surface; the product never calls it.
#include <algorithm>
#include <cmath>
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

// the same with ANY number of input descriptors (names / spans / data: n_desc entries, each span x n column-major) and every descriptor
// of the result handed back: out_desc (capacity out_rows_cap x n floats) receives them one after the other in the container's order,
// each span x n_out, and out_names "name:span;name:span;..." in that order.
int nim_test_filter_chain_descs(icpmi_handle h, const char* yaml_seq, const float* in4, int64_t n, int n_desc, const char* const* names,
                                const int* spans, const float* const* data, float* out4, float* out_desc, int out_rows_cap, char* out_names,
                                int out_names_cap, int64_t* n_out, char* err, int err_cap)
{
    try {
        nim::DataPoints c((size_t)n);
        std::memcpy(c.features.data(), in4, sizeof(float) * 4 * (size_t)n);
        for (int d = 0; d < n_desc; ++d) c.addDescriptor(names[d], spans[d], std::vector<float>(data[d], data[d] + (size_t)spans[d] * n));
        nim::DataPointsFilters chain(nim::yaml::Load(yaml_seq), h);
        chain.apply(c);
        const size_t m = c.getNbPoints();
        std::memcpy(out4, c.features.data(), sizeof(float) * 4 * m);
        std::string all;
        size_t rows = 0;
        for (const auto& d : c.descriptors) {
            if (d.data.size() != (size_t)d.span * m) throw std::logic_error("the filter chain left descriptor " + d.name + " out of step with the points");
            if (rows + (size_t)d.span > (size_t)out_rows_cap) throw std::logic_error("more descriptor rows than the caller has room for");
            std::memcpy(out_desc + rows * m, d.data.data(), sizeof(float) * d.data.size());
            rows += (size_t)d.span;
            all += d.name + ":" + std::to_string(d.span) + ";";
        }
        if (all.size() + 1 > (size_t)out_names_cap) throw std::logic_error("descriptor names do not fit");
        std::memcpy(out_names, all.c_str(), all.size() + 1);
        *n_out = (int64_t)m;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap(map4 + map_normals3), then operator() on the reading (scan4 +
// scan_normals3 as `normals`, may be NULL).  noise (n floats, may be NULL) goes to icpmi_set_reading_sensor_noise right before the
// registration: what a caller without SimpleSensorNoiseDataPointsFilter had to do by hand.  T_out16 column-major, stats_out the
// registration's icpmi_stats.
int nim_test_icp_register(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                          const float* scan_normals3, const float* noise, float* T_out16, icpmi_stats* stats_out, char* err, int err_cap)
{
    try {
        nim::DataPoints map((size_t)m), scan((size_t)n);
        std::memcpy(map.features.data(), map4, sizeof(float) * 4 * (size_t)m);
        if (map_normals3) map.addDescriptor("normals", 3, std::vector<float>(map_normals3, map_normals3 + 3 * (size_t)m));
        std::memcpy(scan.features.data(), scan4, sizeof(float) * 4 * (size_t)n);
        if (scan_normals3) scan.addDescriptor("normals", 3, std::vector<float>(scan_normals3, scan_normals3 + 3 * (size_t)n));
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(map)) throw std::runtime_error("setMap refused the map");
        if (noise) nim::GpuICPSequence::check(icp.handle(), icpmi_set_reading_sensor_noise(icp.handle(), noise, n));
        const nim::Mat4 T = icp(scan);
        std::memcpy(T_out16, T.data(), sizeof(float) * 16);
        *stats_out = icp.stats();
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// parseMatcher on the `matcher:` entry given as YAML text (no GPU, no handle): the fields it sets, and KDTreeVarDistMatcher's descriptor
// name (empty for KDTreeMatcher) in field_out.  Returns 0, or 1 with the exception's text in err.
int nim_test_parse_matcher(const char* yaml_matcher, int* knn, float* epsilon, float* max_dist, int* var_dist, char* field_out, int field_cap,
                           char* err, int err_cap)
{
    try {
        icpmi_config cfg;
        icpmi_config_default(&cfg);
        std::string field;
        nim::parseMatcher(nim::yaml::Load(yaml_matcher), cfg, field);
        *knn = cfg.knn; *epsilon = cfg.epsilon; *max_dist = cfg.max_dist; *var_dist = cfg.var_dist;
        if (field_out && field_cap > 0) { std::strncpy(field_out, field.c_str(), (size_t)field_cap - 1); field_out[field_cap - 1] = 0; }
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// parseErrorMinimizer on the `errorMinimizer:` entry of the ICP chain given as YAML text (no GPU, no handle): the fields it sets and PlaneToPlaneErrorMinimizer's
// epsilon (0.001 unless the entry names one).  Returns 0, or 1 with the exception's text in err.
int nim_test_parse_error_minimizer(const char* yaml_icp, int* minimizer, int* force_4dof, int* force_2d, int* covariance, float* degeneracy_threshold,
                                   float* plane_epsilon, char* err, int err_cap)
{
    try {
        icpmi_config cfg;
        icpmi_config_default(&cfg);
        float eps = 1e-3f;
        int model = ICPMI_PLANE_MODEL_GICP;
        nim::parseErrorMinimizer(nim::yaml::Load(yaml_icp)["errorMinimizer"], cfg, eps, model);
        *minimizer = cfg.minimizer; *force_4dof = cfg.force_4dof; *force_2d = cfg.force_2d; *covariance = cfg.covariance;
        *degeneracy_threshold = cfg.degeneracy_threshold; *plane_epsilon = eps;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// the matcher, the number of outlier filters and the error minimiser of an ICP chain given as YAML text, as loadFromYamlNode reads them for
// VoxelMatcher (no GPU, no handle): its voxel size (0 for another matcher) and the minimiser.  Returns 0, or 1 with the exception's text in err.
int nim_test_parse_voxel_chain(const char* yaml_icp, float* voxel_size, int* minimizer, int* plane_model, char* err, int err_cap)
{
    try {
        icpmi_config cfg;
        icpmi_config_default(&cfg);
        const nim::yaml::Node icp = nim::yaml::Load(yaml_icp);
        std::string field;
        float size = 0.f, eps = 1e-3f;
        int model = ICPMI_PLANE_MODEL_GICP;
        if (icp["matcher"]) nim::parseMatcher(icp["matcher"], cfg, field, &size);
        const int n_out = icp["outlierFilters"].IsSequence() ? (int)icp["outlierFilters"].seq.size() : 0;
        if (icp["errorMinimizer"]) nim::parseErrorMinimizer(icp["errorMinimizer"], cfg, eps, model);
        nim::checkVoxelChain(size, n_out, cfg.minimizer, model);
        *voxel_size = size; *minimizer = cfg.minimizer; *plane_model = model;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// ... and the photometric term of IntensityPointToPlaneErrorMinimizer with it (weight 0, knn 10 and an empty name under every other entry)
int nim_test_parse_error_minimizer_intensity(const char* yaml_icp, int* minimizer, int* force_4dof, float* weight, int* knn, char* desc_name, int desc_cap,
                                             char* err, int err_cap)
{
    try {
        icpmi_config cfg;
        icpmi_config_default(&cfg);
        float eps = 1e-3f;
        int model = ICPMI_PLANE_MODEL_GICP;
        nim::IntensityTerm term;
        nim::parseErrorMinimizer(nim::yaml::Load(yaml_icp)["errorMinimizer"], cfg, eps, model, &term);
        *minimizer = cfg.minimizer; *force_4dof = cfg.force_4dof; *weight = term.weight; *knn = term.knn;
        if (desc_name && desc_cap > 0) { std::strncpy(desc_name, term.descName.c_str(), (size_t)desc_cap - 1); desc_name[desc_cap - 1] = 0; }
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// ... and the pair model of ICPMI_MIN_PLANE_TO_PLANE with it (ICPMI_PLANE_MODEL_*: SymmetricPointToPlaneErrorMinimizer names the symmetric one)
int nim_test_parse_error_minimizer_model(const char* yaml_icp, int* minimizer, int* force_4dof, float* plane_epsilon, int* plane_model,
                                         char* err, int err_cap)
{
    try {
        icpmi_config cfg;
        icpmi_config_default(&cfg);
        float eps = 1e-3f;
        int model = ICPMI_PLANE_MODEL_GICP;
        nim::parseErrorMinimizer(nim::yaml::Load(yaml_icp)["errorMinimizer"], cfg, eps, model);
        *minimizer = cfg.minimizer; *force_4dof = cfg.force_4dof; *plane_epsilon = eps; *plane_model = model;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// nim::deskewSweep (what Mapper::deskew runs on its own handle) on handle h.  The cloud: in4 + n_desc float descriptors (names / spans /
// data, each span x n column-major) + one optional int64 row group (time_name / times, one row; may be NULL).  The motion: n_poses
// stamps (ns) and poses (7 doubles each); stamp_ns the scan's stamp.  Back come out4, every descriptor in nim_test_filter_chain_descs'
// layout and the time row (out_times, may be NULL).  Returns 0; 2 with the text in err for an InvalidField; 1 for any other exception.
int nim_test_deskew(icpmi_handle h, const float* in4, int64_t n, int n_desc, const char* const* names, const int* spans, const float* const* data,
                    const char* time_name, const int64_t* times, int n_poses, const int64_t* pose_stamp_ns, const double* pose7, int64_t stamp_ns,
                    const char* time_field, double time_unit, int64_t round_to_ns, int extrapolate, float* out4, float* out_desc,
                    int out_rows_cap, char* out_names, int out_names_cap, int64_t* out_times, char* err, int err_cap)
{
    const auto fail = [&](const std::exception& e, int rc) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return rc;
    };
    try {
        nim::DataPoints c((size_t)n);
        std::memcpy(c.features.data(), in4, sizeof(float) * 4 * (size_t)n);
        for (int d = 0; d < n_desc; ++d) c.addDescriptor(names[d], spans[d], std::vector<float>(data[d], data[d] + (size_t)spans[d] * n));
        if (time_name && times) c.addTime(time_name, 1, std::vector<int64_t>(times, times + (size_t)n));
        nim::SweepMotion motion;
        for (int k = 0; k < n_poses; ++k) {
            motion.stampNs.push_back(pose_stamp_ns[k]);
            std::array<double, 7> p;
            std::memcpy(p.data(), pose7 + 7 * (size_t)k, sizeof p);
            motion.pose.push_back(p);
        }
        nim::DeskewOptions opts;
        opts.timeField = time_field; opts.timeUnit = time_unit; opts.roundToNs = round_to_ns; opts.extrapolate = extrapolate != 0;
        nim::deskewSweep(h, c, motion, nim::TimePoint{std::chrono::nanoseconds(stamp_ns)}, opts);
        if (c.getNbPoints() != (size_t)n) throw std::logic_error("deskewing changed the number of points");
        std::memcpy(out4, c.features.data(), sizeof(float) * 4 * (size_t)n);
        std::string all;
        size_t rows = 0;
        for (const auto& d : c.descriptors) {
            if (d.data.size() != (size_t)d.span * n) throw std::logic_error("deskewing left descriptor " + d.name + " out of step with the points");
            if (rows + (size_t)d.span > (size_t)out_rows_cap) throw std::logic_error("more descriptor rows than the caller has room for");
            std::memcpy(out_desc + rows * (size_t)n, d.data.data(), sizeof(float) * d.data.size());
            rows += (size_t)d.span;
            all += d.name + ":" + std::to_string(d.span) + ";";
        }
        if (all.size() + 1 > (size_t)out_names_cap) throw std::logic_error("descriptor names do not fit");
        std::memcpy(out_names, all.c_str(), all.size() + 1);
        if (time_name && out_times && c.timeExists(time_name)) std::memcpy(out_times, c.getTimeByName(time_name).data.data(), sizeof(int64_t) * (size_t)n);
        return 0;
    } catch (const nim::InvalidField& e) {
        return fail(e, 2);
    } catch (const std::exception& e) {
        return fail(e, 1);
    }
}

// The arithmetic of icpmi_deskew as one host thread runs it, float32, from the table icpmi_deskew_table builds: what a caller without the
// device pass has to do, and the point of comparison of scripts/deskew_bench.py.  Times are taken as valid (no NaN, inside the stamps
// or clamped to them); no handle, no GPU.  Returns 0, or 1 with the library's message in err.
int nim_test_deskew_host_loop(const float* in4, int64_t n, const float* t_rel, const icpmi_sweep_motion* m, float* out4, char* err, int err_cap)
{
    const int K = m->n_poses;
    std::vector<float> q(4 * (size_t)std::max(K, 2)), p(3 * q.size() / 4), om(q.size() / 4), is(q.size() / 4);
    if (icpmi_deskew_table(m, q.data(), p.data(), om.data(), is.data()) != ICPMI_OK) {
        if (err && err_cap > 0) { std::strncpy(err, icpmi_last_error(nullptr), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
    const double* s = m->stamp_s;
    for (int64_t i = 0; i < n; ++i) {
        double tau = (double)t_rel[i] * m->time_unit_s;
        if (m->round_s > 0.0) tau = std::rint(tau / m->round_s) * m->round_s;
        tau = std::min(std::max(tau, s[0]), s[K - 1]);
        int lo = 0, hi = K - 1;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s[mid] <= tau) lo = mid; else hi = mid; }
        const float u = (float)((tau - s[lo]) / (s[lo + 1] - s[lo])), um = 1.0f - u;
        float w0 = um, w1 = u;
        if (is[lo] != 0.0f) { w0 = std::sin(um * om[lo]) * is[lo]; w1 = std::sin(u * om[lo]) * is[lo]; }
        const float* qa = &q[4 * (size_t)lo]; const float* pa = &p[3 * (size_t)lo];
        const float qx = w0 * qa[0] + w1 * qa[4], qy = w0 * qa[1] + w1 * qa[5], qz = w0 * qa[2] + w1 * qa[6], qw = w0 * qa[3] + w1 * qa[7];
        const float px = um * pa[0] + u * pa[3], py = um * pa[1] + u * pa[4], pz = um * pa[2] + u * pa[5];
        const float xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
        const float* x = in4 + 4 * i; float* o = out4 + 4 * i;
        o[0] = (((1.0f - 2.0f * (yy + zz)) * x[0] + (2.0f * (xy - wz)) * x[1]) + (2.0f * (xz + wy)) * x[2]) + px;
        o[1] = (((2.0f * (xy + wz)) * x[0] + (1.0f - 2.0f * (xx + zz)) * x[1]) + (2.0f * (yz - wx)) * x[2]) + py;
        o[2] = (((2.0f * (xz - wy)) * x[0] + (2.0f * (yz + wx)) * x[1]) + (1.0f - 2.0f * (xx + yy)) * x[2]) + pz;
        o[3] = x[3];
    }
    return 0;
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

// The same replay, handing back the map it built instead of the covariances: out4 (capacity cap points) the mapper's map, out_desc /
// out_names every descriptor of it in nim_test_filter_chain_descs' layout, *map_updates how many scans started a map update and
// *resident_updates Map::residentUpdateCount() -- how many of those ran on the resident map (tests/test_gpu_max_density.py).
int nim_test_mapper_replay_map(const char* config, int n_scans, const char* const* paths, const float* poses16, const int64_t* stamps_ns,
                               float* poses_out16, float* out4, int64_t cap, float* out_desc, int out_rows_cap, char* out_names, int out_names_cap,
                               int64_t* n_out, int64_t* map_updates, int64_t* resident_updates, char* err, int err_cap)
{
    try {
        nim::Mapper mapper(config, true, false, true, false);
        *map_updates = 0;
        for (int i = 0; i < n_scans; ++i) {
            nim::DataPoints cloud = nim::DataPoints::load(paths[i]);
            mapper.applyInputFilters(cloud);
            nim::Mat4 pose;
            std::memcpy(pose.data(), poses16 + 16 * i, sizeof(float) * 16);
            mapper.processInput(cloud, pose, nim::TimePoint{std::chrono::nanoseconds(stamps_ns[i])});
            std::memcpy(poses_out16 + 16 * i, mapper.getPose().data(), sizeof(float) * 16);
            if (mapper.lastScanStartedMapUpdate()) ++*map_updates;
        }
        *resident_updates = mapper.residentMapUpdates();
        const nim::DataPoints c = mapper.getMap();
        const size_t m = c.getNbPoints();
        if ((int64_t)m > cap) throw std::logic_error("the map is larger than the caller has room for");
        std::memcpy(out4, c.features.data(), sizeof(float) * 4 * m);
        std::string all;
        size_t rows = 0;
        for (const auto& d : c.descriptors) {
            if (d.data.size() != (size_t)d.span * m) throw std::logic_error("descriptor " + d.name + " is out of step with the points");
            if (rows + (size_t)d.span > (size_t)out_rows_cap) throw std::logic_error("more descriptor rows than the caller has room for");
            std::memcpy(out_desc + rows * m, d.data.data(), sizeof(float) * d.data.size());
            rows += (size_t)d.span;
            all += d.name + ":" + std::to_string(d.span) + ";";
        }
        if (all.size() + 1 > (size_t)out_names_cap) throw std::logic_error("descriptor names do not fit");
        std::memcpy(out_names, all.c_str(), all.size() + 1);
        *n_out = (int64_t)m;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// GpuICPSequence on device 0: loadFromYamlNode(yaml_icp), setMap(map4 + map_normals3), then -- T16 == NULL -- operator() on the reading
// (scan4 + scan_normals3 as `normals`, may be NULL) and residual(reading, T of that registration, kind); with T16 (column-major) no
// registration, residual(reading, T16, kind).  *out the icpmi_residual, T_out16 the T used, *residual_error_out what
// errorMinimizer->getResidualError(reading, T) returns (kind 0 only; else the same sum).  Returns 0; 2 ConvergenceError, 3 InvalidField,
// 4 InvalidParameter, 1 any other exception, the text in err.
int nim_test_icp_residual(const char* yaml_icp, const float* map4, int64_t m, const float* map_normals3, const float* scan4, int64_t n,
                          const float* scan_normals3, const float* T16, int kind, icpmi_residual* out, float* T_out16,
                          float* residual_error_out, char* err, int err_cap)
{
    const auto fail = [&](const std::exception& e, int rc) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return rc;
    };
    try {
        nim::DataPoints map((size_t)m), scan((size_t)n);
        std::memcpy(map.features.data(), map4, sizeof(float) * 4 * (size_t)m);
        if (map_normals3) map.addDescriptor("normals", 3, std::vector<float>(map_normals3, map_normals3 + 3 * (size_t)m));
        std::memcpy(scan.features.data(), scan4, sizeof(float) * 4 * (size_t)n);
        if (scan_normals3) scan.addDescriptor("normals", 3, std::vector<float>(scan_normals3, scan_normals3 + 3 * (size_t)n));
        nim::GpuICPSequence icp(0);
        icp.loadFromYamlNode(nim::yaml::Load(yaml_icp));
        if (!icp.setMap(map)) throw std::runtime_error("setMap refused the map");
        nim::Mat4 T;
        if (T16) std::memcpy(T.data(), T16, sizeof(float) * 16);
        else T = icp(scan);
        *out = icp.residual(scan, T, kind);
        std::memcpy(T_out16, T.data(), sizeof(float) * 16);
        *residual_error_out = kind == ICPMI_RES_CHAIN ? icp.errorMinimizer->getResidualError(scan, T) : (float)out->sum_abs;
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2);
    } catch (const nim::InvalidField& e) {
        return fail(e, 3);
    } catch (const nim::InvalidParameter& e) {
        return fail(e, 4);
    } catch (const std::exception& e) {
        return fail(e, 1);
    }
}

// The offline replay of nim_test_mapper_replay with Mapper::setScoreRegistrations(score).  freeze_after_first: the mapper stops mapping
// behind the first scan, so that every later scan registers against the map that scan built.  After every processInput: the pose,
// lastResidualValid() / lastResidual(), and -- by_hand != NULL and the scan was scored -- GpuICPSequence::residual called by hand on the
// same filtered scan moved by the same prior, under Mapper::lastCorrection() (the map must not have changed in between: freeze).
int nim_test_mapper_replay_scored(const char* config, int n_scans, const char* const* paths, const float* poses16, const int64_t* stamps_ns,
                                  int score, int freeze_after_first, float* poses_out16, icpmi_residual* res_out, int32_t* res_valid,
                                  icpmi_residual* by_hand, char* err, int err_cap)
{
    try {
        nim::Mapper mapper(config, true, false, true, false);
        mapper.setScoreRegistrations(score != 0);
        for (int i = 0; i < n_scans; ++i) {
            nim::DataPoints cloud = nim::DataPoints::load(paths[i]);
            mapper.applyInputFilters(cloud);
            nim::Mat4 pose;
            std::memcpy(pose.data(), poses16 + 16 * i, sizeof(float) * 16);
            mapper.processInput(cloud, pose, nim::TimePoint{std::chrono::nanoseconds(stamps_ns[i])});
            std::memcpy(poses_out16 + 16 * i, mapper.getPose().data(), sizeof(float) * 16);
            res_valid[i] = mapper.lastResidualValid() ? 1 : 0;
            res_out[i] = mapper.lastResidual();
            if (by_hand) {
                std::memset(by_hand + i, 0, sizeof *by_hand);
                if (mapper.lastResidualValid()) {
                    const nim::DataPoints inMap = nim::RigidTransformation(mapper.icpSequence().handle()).compute(cloud, pose);
                    by_hand[i] = mapper.icpSequence().residual(inMap, mapper.lastCorrection());
                }
            }
            if (i == 0 && freeze_after_first) mapper.setIsMapping(false);
        }
        return 0;
    } catch (const std::exception& e) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return 1;
    }
}

// Mapper::processSweep scan by scan on an offline mapper built from `config`: scan i is scans4[i] (ns[i] points, sensor frame, skewed) with
// its point times t_rel[i] as the float descriptor `t` (nanoseconds from the stamp), the priors priors_begin16 / priors_end16 (column-major,
// 16 floats per scan), the sweep spanning [begin_s, end_s].  Back per scan: the two poses processSweep returned, the icpmi_sweep_result, the
// mapper's pose (getPose()) and the size of its map after the call.  Returns 0; 2 ConvergenceError, 3 InvalidField, 4 InvalidParameter, 1
// any other exception, the text in err.
int nim_test_mapper_sweep(const char* config, int n_scans, const float* const* scans4, const int64_t* ns, const float* const* t_rel,
                          const float* priors_begin16, const float* priors_end16, const int64_t* stamps_ns, double begin_s, double end_s,
                          int max_iterations, float* begin_out16, float* end_out16, icpmi_sweep_result* res_out, float* pose_out16,
                          int64_t* map_sizes, char* err, int err_cap)
{
    const auto fail = [&](const std::exception& e, int rc) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return rc;
    };
    try {
        nim::Mapper mapper(config, true, false, true, false);
        nim::SweepOptions opts;
        opts.beginS = begin_s; opts.endS = end_s; opts.maxIterations = max_iterations;
        for (int i = 0; i < n_scans; ++i) {
            const size_t n = (size_t)ns[i];
            nim::DataPoints cloud(n);
            std::memcpy(cloud.features.data(), scans4[i], sizeof(float) * 4 * n);
            cloud.addDescriptor("t", 1, std::vector<float>(t_rel[i], t_rel[i] + n));
            nim::Mat4 pb, pe;
            std::memcpy(pb.data(), priors_begin16 + 16 * i, sizeof(float) * 16);
            std::memcpy(pe.data(), priors_end16 + 16 * i, sizeof(float) * 16);
            const nim::SweepRegistration reg = mapper.processSweep(cloud, pb, pe, nim::TimePoint{std::chrono::nanoseconds(stamps_ns[i])}, opts);
            std::memcpy(begin_out16 + 16 * i, reg.begin.data(), sizeof(float) * 16);
            std::memcpy(end_out16 + 16 * i, reg.end.data(), sizeof(float) * 16);
            res_out[i] = reg.stats;
            std::memcpy(pose_out16 + 16 * i, mapper.getPose().data(), sizeof(float) * 16);
            map_sizes[i] = (int64_t)mapper.getMap().getNbPoints();
        }
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2);
    } catch (const nim::InvalidField& e) {
        return fail(e, 3);
    } catch (const nim::InvalidParameter& e) {
        return fail(e, 4);
    } catch (const std::exception& e) {
        return fail(e, 1);
    }
}

// Mapper::processInput scan by scan on an offline mapper built from `config`: scan i is scans4[i] (ns[i] points, sensor frame) with the 1-row
// descriptor `desc_name` = descs[i], under the prior poses16 (column-major, 16 floats per scan).  Back per scan: the mapper's pose, the size
// of its map after the call and whether that map carries the descriptor.  Returns 0; 2 ConvergenceError, 3 InvalidField, 4 InvalidParameter,
// 1 any other exception, the text in err.
int nim_test_mapper_descriptor_scans(const char* config, int n_scans, const float* const* scans4, const int64_t* ns, const char* desc_name,
                                     const float* const* descs, const float* poses16, const int64_t* stamps_ns, float* pose_out16, int64_t* map_sizes,
                                     int* map_has_desc, char* err, int err_cap)
{
    const auto fail = [&](const std::exception& e, int rc) {
        if (err && err_cap > 0) { std::strncpy(err, e.what(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
        return rc;
    };
    try {
        nim::Mapper mapper(config, true, false, true, false);
        for (int i = 0; i < n_scans; ++i) {
            const size_t n = (size_t)ns[i];
            nim::DataPoints cloud(n);
            std::memcpy(cloud.features.data(), scans4[i], sizeof(float) * 4 * n);
            cloud.addDescriptor(desc_name, 1, std::vector<float>(descs[i], descs[i] + n));
            nim::Mat4 prior;
            std::memcpy(prior.data(), poses16 + 16 * i, sizeof(float) * 16);
            mapper.processInput(cloud, prior, nim::TimePoint{std::chrono::nanoseconds(stamps_ns[i])});
            std::memcpy(pose_out16 + 16 * i, mapper.getPose().data(), sizeof(float) * 16);
            const nim::DataPoints map = mapper.getMap();
            map_sizes[i] = (int64_t)map.getNbPoints();
            map_has_desc[i] = map.descriptorExists(desc_name) ? 1 : 0;
        }
        return 0;
    } catch (const nim::ConvergenceError& e) {
        return fail(e, 2);
    } catch (const nim::InvalidField& e) {
        return fail(e, 3);
    } catch (const nim::InvalidParameter& e) {
        return fail(e, 4);
    } catch (const std::exception& e) {
        return fail(e, 1);
    }
}

} // extern "C"
