// IcpSequence.cpp -- see IcpSequence.h.
#include "IcpSequence.h"

#include <cstdlib>

#include <algorithm>
#include <cmath>
#include <limits>
#include <cstring>

namespace nim {

void GpuICPSequence::check(icpmi_handle h, icpmi_status s)
{
    if (s == ICPMI_OK) return;
    const std::string msg = icpmi_last_error(h);
    switch (s) {
        case ICPMI_ERR_NO_POINT_TO_MINIMIZE:
        case ICPMI_ERR_NO_OUTLIER_TO_FILTER:
        case ICPMI_ERR_BOUND:
        case ICPMI_ERR_NAN: throw ConvergenceError(msg);
        case ICPMI_ERR_MISSING_NORMALS: throw InvalidField(msg);
        case ICPMI_ERR_INVALID_ARG: throw InvalidParameter(msg);
        default: throw std::runtime_error(msg);
    }
}

// the covariance of the registration that just ran, read before anything else (a map update) reuses the matcher's buffers
void GpuICPSequence::keepCovariance()
{
    haveCovariance = cfg.covariance != 0 && icpmi_get_covariance(h, covariance.data()) == ICPMI_OK;
    haveLocalizability = cfg.degeneracy_threshold != 0.f && icpmi_get_localizability(h, &localizability) == ICPMI_OK;
}

icpmi_localizability GpuICPSequence::ErrorMinimizerView::getLocalizability() const
{
    if (owner->haveLocalizability) return owner->localizability;
    icpmi_localizability r{};
    check(owner->h, icpmi_get_localizability(owner->h, &r)); // (throws: nothing to read)
    return r;
}

std::array<float, 36> GpuICPSequence::ErrorMinimizerView::getCovariance() const
{
    if (owner->haveCovariance) return owner->covariance;
    std::array<float, 36> c{};
    check(owner->h, icpmi_get_covariance(owner->h, c.data())); // (throws: nothing to read)
    return c;
}

GpuICPSequence::GpuICPSequence(int device)
{
    icpmi_config_default(&cfg);
    cfg.device = device;
    recreate();
}

GpuICPSequence::~GpuICPSequence() { icpmi_destroy(h); }

// the mapper's is3D == false (Mapper.h:53): every cloud is planar (z == 0); kept across loadFromYamlNode / setDefault
void GpuICPSequence::setPlanar(bool on)
{
    planar = on;
    cfg.is_2d = on ? 1 : 0;
    recreate();
}

// icpmi_set_voxel_matcher: the voxel size of VoxelMatcher (0: off); handle state, kept across setPlanar
void GpuICPSequence::setVoxelMatcher(float size)
{
    check(h, icpmi_set_voxel_matcher(h, size));
    voxelSize = size;
    voxelSizes.clear();
}

// icpmi_set_voxel_schedule: 1 to 4 voxel sizes, strictly descending (an empty list: off); handle state like setVoxelMatcher
void GpuICPSequence::setVoxelSchedule(const std::vector<float>& sizes)
{
    check(h, icpmi_set_voxel_schedule(h, sizes.data(), (int32_t)sizes.size()));
    voxelSizes = sizes;
    voxelSize = sizes.empty() ? 0.f : sizes.back();
}

// icpmi_get_voxel_schedule_report of the last registration: one entry per level entered
std::vector<GpuICPSequence::VoxelLevelReport> GpuICPSequence::voxelScheduleReport() const
{
    int32_t levels = 0, it[4], pf[4], pl[4];
    check(h, icpmi_get_voxel_schedule_report(h, &levels, it, pf, pl));
    std::vector<VoxelLevelReport> out;
    for (int l = 0; l < levels && l < 4; ++l) out.push_back({it[l], pf[l], pl[l]});
    return out;
}

void GpuICPSequence::recreate()
{
    // the handle is created once and re-configured afterwards: filters, modules and transformations
    // created from it keep a valid GPU context across loadFromYamlNode / setDefault
    if (h) check(h, icpmi_set_config(h, &cfg));
    else check(nullptr, icpmi_create(&cfg, &h));
}

void GpuICPSequence::setDefault()
{
    // libpointmatcher's default chain (PM::ICPChainBase::setDefault, called at Mapper.cpp:77 when the configuration has no
    // `icp:` key): RandomSampling(0.75) on the reading, SamplingSurfaceNormal on the reference,
    // KDTreeMatcher knn 1, TrimmedDist 0.85, PointToPlane, Counter 40 + Differential(1e-3, 1e-3, 3).
    const int dev = cfg.device;
    icpmi_config_default(&cfg);
    cfg.device = dev;
    cfg.is_2d = planar ? 1 : 0;
    genericDescName.clear(); genericReadDescName.clear(); maxDistFieldName.clear();
    intensity = IntensityTerm{};
    cfg.n_outlier = 1;
    cfg.outlier[0].type = ICPMI_OUT_TRIMMEDDIST;
    cfg.outlier[0].param = 0.85f;
    cfg.minimizer = ICPMI_MIN_POINT_TO_PLANE;
    cfg.use_differential = 1;
    recreate();
    check(h, icpmi_set_intensity_weight(h, 0.f)); // (handle state, which icpmi_set_config leaves: a chain loaded before may have set it)
    voxelSize = 0.f; voxelSizes.clear();
    check(h, icpmi_set_voxel_matcher(h, 0.f));    // (likewise)
    readingDataPointsFilters = std::make_shared<DataPointsFilters>();
    readingDataPointsFilters->ctx = h;
    readingDataPointsFilters->filters.push_back(createDataPointsFilter("RandomSamplingDataPointsFilter", yaml::Node(), h));
    referenceDataPointsFilters = std::make_shared<DataPointsFilters>();
    referenceDataPointsFilters->ctx = h;
    referenceDataPointsFilters->filters.push_back(createDataPointsFilter("SamplingSurfaceNormalDataPointsFilter", yaml::Node(), h));
    readingStepDataPointsFilters.reset();
}

void requireKnown(const yaml::Node& params, std::initializer_list<const char*> known, const std::string& who)
{
    if (!params.IsMap()) return;
    for (const auto& kv : params.map) {
        bool ok = false;
        for (const char* k : known) ok |= kv.first == k;
        if (!ok) throw InvalidParameter(who + ": unknown parameter " + kv.first);
    }
}

std::pair<std::string, yaml::Node> singleEntry(const yaml::Node& n, const std::string& what)
{
    if (n.IsScalar()) return {n.scalar, yaml::Node()};
    if (n.IsMap() && n.map.size() == 1) return {n.map[0].first, n.map[0].second};
    throw InvalidParameter("malformed " + what + " entry");
}

// the `matcher:` entry of an ICP chain into the configuration; maxDistField = KDTreeVarDistMatcher's descriptor name, empty for KDTreeMatcher
void parseMatcher(const yaml::Node& matcher, icpmi_config& cfg, std::string& maxDistField, float* voxelSize, std::vector<float>* voxelSizes)
{
    maxDistField.clear();
    cfg.var_dist = 0;
    if (voxelSize) *voxelSize = 0.f;
    if (voxelSizes) voxelSizes->clear();
    auto e = singleEntry(matcher, "matcher");
    if (e.first == "VoxelMatcher") {
        // voxelised plane-to-plane ICP (not libpointmatcher's; include/icpmi.h: icpmi_set_voxel_matcher): a reading point is paired with the
        // map voxel it falls into -- no search, hence no knn / maxDist / epsilon
        requireKnown(e.second, {"voxelSize", "voxelSizes"}, "VoxelMatcher");
        if (e.second["voxelSize"] && e.second["voxelSizes"])
            throw InvalidParameter("VoxelMatcher: voxelSize and voxelSizes are one parameter said two ways: give one of them");
        float size = 1.f;
        if (e.second["voxelSizes"]) {
            // a schedule, coarsest first: the rules of icpmi_set_voxel_schedule (include/icpmi.h)
            const yaml::Node& list = e.second["voxelSizes"];
            if (!list.IsSequence() || list.seq.empty() || list.seq.size() > 4) throw InvalidParameter("VoxelMatcher: voxelSizes takes 1 to 4 voxel sizes");
            if (!voxelSizes) throw InvalidParameter("VoxelMatcher: voxelSizes is not available here");
            for (const yaml::Node& item : list.seq) {
                const float v = item.as<float>();
                if (!std::isfinite(v) || !(v > 0.f)) throw InvalidParameter("VoxelMatcher: every voxel size of voxelSizes must be finite and > 0");
                if (!voxelSizes->empty() && !(v < voxelSizes->back())) throw InvalidParameter("VoxelMatcher: voxelSizes must be strictly descending (coarsest first)");
                voxelSizes->push_back(v);
            }
            size = voxelSizes->back();
        } else {
            size = e.second["voxelSize"] ? e.second["voxelSize"].as<float>() : 1.f;
            if (!std::isfinite(size) || !(size > 0.f)) throw InvalidParameter("VoxelMatcher: voxelSize must be finite and > 0");
        }
        if (!voxelSize) throw InvalidParameter("VoxelMatcher: not available here");
        *voxelSize = size;
        // the loop reads none of KDTreeMatcher's parameters; getResidualError, which scores the pose through the nearest-neighbour matcher,
        // runs it with that matcher's defaults whatever an earlier chain left in cfg
        icpmi_config def;
        icpmi_config_default(&def);
        cfg.knn = def.knn; cfg.epsilon = def.epsilon; cfg.epsilon_approx = def.epsilon_approx; cfg.max_dist = def.max_dist;
        return;
    }
    if (e.first == "KDTreeVarDistMatcher") {
        // every reading point searches within its own radius, the reading's 1-row descriptor `maxDistField` (operator() hands it over)
        requireKnown(e.second, {"knn", "epsilon", "searchType", "maxDistField"}, "KDTreeVarDistMatcher");
        cfg.var_dist = 1;
        maxDistField = e.second["maxDistField"] ? e.second["maxDistField"].as<std::string>() : std::string("maxSearchDist");
    } else {
        if (e.first != "KDTreeMatcher") throw InvalidParameter("unknown matcher " + e.first);
        requireKnown(e.second, {"knn", "epsilon", "searchType", "maxDist", "maxDistField"}, "KDTreeMatcher");
    }
    if (e.second["knn"]) cfg.knn = e.second["knn"].as<int>();
    if (e.second["epsilon"]) cfg.epsilon = e.second["epsilon"].as<float>();
    // NIM_EPSILON_APPROX=1 (deployment knob): `epsilon` prunes the search as libnabo's maxError2 does (icpmi_config::
    // epsilon_approx); default: the exact search, which is a valid answer for every epsilon
    static const bool approx = [] { const char* v = std::getenv("NIM_EPSILON_APPROX"); return v && std::atoi(v) != 0; }();
    cfg.epsilon_approx = approx ? 1 : 0;
    // NIM_KNN_WG_FROM=n (deployment knob, icpmi_config::knn_wg_from): the first iteration (n - 1) of a k > 1 loop the workgroup-cooperative matcher serves;
    // default 0 = from iteration 2.  Same results either way; which is faster depends on how far the first solve moves the reading
    static const int wgFrom = [] { const char* v = std::getenv("NIM_KNN_WG_FROM"); return v ? std::atoi(v) : 0; }();
    cfg.knn_wg_from = wgFrom;
    if (e.second["maxDist"]) cfg.max_dist = e.second["maxDist"].as<float>();
}

// the `errorMinimizer:` entry of an ICP chain into the configuration; planeEpsilon = PlaneToPlaneErrorMinimizer.epsilon (left alone by the
// others), planeModel = the pair model of ICPMI_MIN_PLANE_TO_PLANE (SymmetricPointToPlaneErrorMinimizer sets it; left alone by the others)
void parseErrorMinimizer(const yaml::Node& node, icpmi_config& cfg, float& planeEpsilon, int& planeModel, IntensityTerm* intensity)
{
    auto e = singleEntry(node, "errorMinimizer");
    if (intensity) *intensity = IntensityTerm{};
    if (e.first == "IdentityErrorMinimizer") cfg.minimizer = ICPMI_MIN_IDENTITY;
    else if (e.first == "PointToPointErrorMinimizer") cfg.minimizer = ICPMI_MIN_POINT_TO_POINT;
    else if (e.first == "PointToPlaneErrorMinimizer" || e.first == "PointToPlaneWithCovErrorMinimizer") {
        cfg.minimizer = ICPMI_MIN_POINT_TO_PLANE;
        if (e.first == "PointToPlaneWithCovErrorMinimizer") { // the same registration, plus getCovariance() (icpmi_get_covariance)
            requireKnown(e.second, {"sensorStdDev", "force2D", "force4DOF", "degeneracyThreshold", "degeneracyAction"}, e.first);
            cfg.covariance = 1;
            if (e.second["sensorStdDev"]) cfg.sensor_std_dev = e.second["sensorStdDev"].as<float>();
        } else requireKnown(e.second, {"force2D", "force4DOF", "degeneracyThreshold", "degeneracyAction"}, e.first); // (a misspelt key must not leave the option off in silence)
        cfg.force_4dof = (e.second["force4DOF"] && e.second["force4DOF"].as<int>() != 0) ? 1 : 0;
        cfg.force_2d = (e.second["force2D"] && e.second["force2D"].as<int>() != 0) ? 1 : 0;
        if (cfg.force_4dof && cfg.force_2d) throw InvalidParameter("PointToPlaneErrorMinimizer: force2D and force4DOF exclude each other");
        // degeneracy-aware solve (not libpointmatcher's): degeneracyThreshold >= 0 (0: off), degeneracyAction constrain | report
        const float thr = e.second["degeneracyThreshold"] ? e.second["degeneracyThreshold"].as<float>() : 0.f;
        const std::string action = e.second["degeneracyAction"] ? e.second["degeneracyAction"].as<std::string>() : std::string("constrain");
        if (!(thr >= 0.f) || !std::isfinite(thr)) throw InvalidParameter(e.first + ": degeneracyThreshold must be finite and >= 0");
        if (action != "constrain" && action != "report") throw InvalidParameter(e.first + ": degeneracyAction must be constrain or report");
        if (thr > 0.f && cfg.force_2d) throw InvalidParameter(e.first + ": degeneracyThreshold and force2D exclude each other");
        cfg.degeneracy_threshold = action == "constrain" ? thr : -thr;
    } else if (e.first == "PlaneToPlaneErrorMinimizer") {
        // generalized ICP from the normals of both clouds (not libpointmatcher's; include/icpmi.h: ICPMI_MIN_PLANE_TO_PLANE)
        requireKnown(e.second, {"epsilon", "force4DOF"}, e.first);
        cfg.minimizer = ICPMI_MIN_PLANE_TO_PLANE;
        cfg.force_4dof = (e.second["force4DOF"] && e.second["force4DOF"].as<int>() != 0) ? 1 : 0;
        if (e.second["epsilon"]) planeEpsilon = e.second["epsilon"].as<float>();
        if (!std::isfinite(planeEpsilon) || !(planeEpsilon > 0.f) || planeEpsilon > 1.f)
            throw InvalidParameter(e.first + ": epsilon must be finite and in (0, 1]");
    } else if (e.first == "SymmetricPointToPlaneErrorMinimizer") {
        // symmetric point-to-plane from the normals of both clouds (not libpointmatcher's; include/icpmi.h: ICPMI_PLANE_MODEL_SYMMETRIC):
        // the plane-to-plane path under its other pair model
        requireKnown(e.second, {"force4DOF"}, e.first);
        cfg.minimizer = ICPMI_MIN_PLANE_TO_PLANE;
        planeModel = ICPMI_PLANE_MODEL_SYMMETRIC;
        cfg.force_4dof = (e.second["force4DOF"] && e.second["force4DOF"].as<int>() != 0) ? 1 : 0;
    } else if (e.first == "IntensityPointToPlaneErrorMinimizer") {
        // point-to-plane with a photometric term from one scalar descriptor of both clouds (not libpointmatcher's; include/icpmi.h:
        // icpmi_set_intensity_weight): the point-to-plane path with a weight on the handle
        requireKnown(e.second, {"lambdaGeometric", "descName", "gradientKnn", "force4DOF"}, e.first);
        cfg.minimizer = ICPMI_MIN_POINT_TO_PLANE;
        cfg.force_4dof = (e.second["force4DOF"] && e.second["force4DOF"].as<int>() != 0) ? 1 : 0;
        IntensityTerm t;
        const float lambda = e.second["lambdaGeometric"] ? e.second["lambdaGeometric"].as<float>() : 0.968f;
        if (!std::isfinite(lambda) || !(lambda > 0.f) || lambda > 1.f) throw InvalidParameter(e.first + ": lambdaGeometric must be finite and in (0, 1]");
        t.weight = 1.f - lambda;
        t.knn = e.second["gradientKnn"] ? e.second["gradientKnn"].as<int>() : 10;
        if (t.knn < 1 || t.knn > 31) throw InvalidParameter(e.first + ": gradientKnn must be in [1, 31]");
        t.descName = e.second["descName"] ? e.second["descName"].str() : std::string("intensity");
        if (t.descName.empty()) throw InvalidParameter(e.first + ": descName must name a descriptor");
        if (intensity) *intensity = t;
    } else throw InvalidParameter("unknown error minimizer " + e.first);
}

// VoxelMatcher is accepted with PlaneToPlaneErrorMinimizer and an empty outlier list only -- the C call's wording (csrc/api.hip: voxel_check)
void checkVoxelChain(float voxelSize, int nOutlier, int minimizer, int planeModel)
{
    if (!(voxelSize > 0.f)) return;
    const std::string who = "register: the voxel matcher (icpmi_set_voxel_matcher > 0) ";
    if (nOutlier > 0)
        throw InvalidParameter(who + "is not served with outlier filters (a pair is a point and the voxel it falls into: there is no match distance to filter on)");
    if (minimizer == ICPMI_MIN_PLANE_TO_PLANE && planeModel != ICPMI_PLANE_MODEL_GICP)
        throw InvalidParameter(who + "is not served with the symmetric pair model (SymmetricPointToPlaneErrorMinimizer)");
    if (minimizer != ICPMI_MIN_PLANE_TO_PLANE) throw InvalidParameter(who + "is defined on PlaneToPlaneErrorMinimizer only");
}

void GpuICPSequence::loadFromYamlNode(const yaml::Node& icp)
{
    const int dev = cfg.device;
    icpmi_config_default(&cfg);
    planeEpsilon = 1e-3f; // PlaneToPlaneErrorMinimizer.epsilon
    planeModel = ICPMI_PLANE_MODEL_GICP; // (SymmetricPointToPlaneErrorMinimizer: the other one)
    cfg.device = dev;
    cfg.is_2d = planar ? 1 : 0;
    if (icp.IsMap())
        for (const auto& kv : icp.map) {
            static const char* valid[] = {"matcher", "outlierFilters", "errorMinimizer", "transformationCheckers", "inspector", "logger",
                                          "readingDataPointsFilters", "referenceDataPointsFilters", "readingStepDataPointsFilters"};
            bool ok = false;
            for (const char* v : valid) ok |= kv.first == v;
            if (!ok) throw InvalidParameter("unknown ICP chain key: " + kv.first);
        }

    maxDistFieldName.clear();
    voxelSize = 0.f;
    voxelSizes.clear();
    if (icp["matcher"]) parseMatcher(icp["matcher"], cfg, maxDistFieldName, &voxelSize, &voxelSizes);
    cfg.n_outlier = 0;
    genericDescName.clear(); genericReadDescName.clear();
    if (icp["outlierFilters"].IsSequence())
        for (const auto& item : icp["outlierFilters"].seq) {
            auto e = singleEntry(item, "outlier filter");
            icpmi_outlier o{};
            auto param = [&](const char* key, float def) {
                requireKnown(e.second, {key}, e.first);
                return e.second[key] ? e.second[key].as<float>() : def;
            };
            if (e.first == "TrimmedDistOutlierFilter") { o.type = ICPMI_OUT_TRIMMEDDIST; o.param = param("ratio", 0.85f); }
            else if (e.first == "MaxDistOutlierFilter") { o.type = ICPMI_OUT_MAXDIST; o.param = param("maxDist", 1.f); }
            else if (e.first == "MinDistOutlierFilter") { o.type = ICPMI_OUT_MINDIST; o.param = param("minDist", 1.f); }
            else if (e.first == "MedianDistOutlierFilter") { o.type = ICPMI_OUT_MEDIANDIST; o.param = param("factor", 3.f); }
            else if (e.first == "SurfaceNormalOutlierFilter") { o.type = ICPMI_OUT_SURFACENORMAL; o.param = param("maxAngle", 1.57f); }
            else if (e.first == "VarTrimmedDistOutlierFilter") {
                // defaults of upstream's registrar: minRatio 0.05, maxRatio 0.99, lambda 0.95
                const yaml::Node& p = e.second;
                requireKnown(p, {"minRatio", "maxRatio", "lambda"}, e.first);
                o.type = ICPMI_OUT_VARTRIMMEDDIST;
                o.param = p["minRatio"] ? p["minRatio"].as<float>() : 0.05f;
                o.param2 = p["maxRatio"] ? p["maxRatio"].as<float>() : 0.99f;
                o.param3 = p["lambda"] ? p["lambda"].as<float>() : 0.95f;
            }
            else if (e.first == "GenericDescriptorOutlierFilter") {
                // defaults of upstream's registrar: source reference, descName none, useSoftThreshold 0, useLargerThan 1, threshold 0.1
                const yaml::Node& p = e.second;
                requireKnown(p, {"source", "descName", "useSoftThreshold", "useLargerThan", "threshold"}, e.first);
                const std::string source = p["source"] ? p["source"].str() : "reference";
                if (source != "reference" && source != "reading") throw InvalidParameter("GenericDescriptorOutlierFilter: source must be reference or reading");
                const std::string name = p["descName"] ? p["descName"].str() : "none";
                if (source == "reading") {
                    // (r4) the descriptor of the READING point decides: its row rides to the device ahead of every registration (operator())
                    if (!genericReadDescName.empty() && genericReadDescName != name) throw InvalidParameter("GenericDescriptorOutlierFilter: one reading descriptor per chain");
                    genericReadDescName = name;
                } else {
                    if (!genericDescName.empty() && genericDescName != name) throw InvalidParameter("GenericDescriptorOutlierFilter: the device tracks one scalar descriptor of the map");
                    genericDescName = name;
                }
                o.type = ICPMI_OUT_GENERICDESCRIPTOR;
                o.param = p["threshold"] ? p["threshold"].as<float>() : 0.1f;
                o.iparam = ((p["useSoftThreshold"] && p["useSoftThreshold"].as<int>()) ? ICPMI_GEN_SOFT : 0) |
                           ((!p["useLargerThan"] || p["useLargerThan"].as<int>()) ? ICPMI_GEN_LARGER : 0) | (source == "reading" ? ICPMI_GEN_SOURCE_READING : 0);
            } else if (e.first == "RobustOutlierFilter") {
                // defaults: robustFct cauchy, tuning 1, scaleEstimator mad, nbIterationForScale 0, distanceType point2point, approximation inf
                const yaml::Node& p = e.second;
                requireKnown(p, {"robustFct", "tuning", "scaleEstimator", "nbIterationForScale", "distanceType", "approximation"}, e.first);
                static const char* fcts[] = {"cauchy", "welsch", "sc", "gm", "tukey", "huber", "L1", "student"};
                const std::string fct = p["robustFct"] ? p["robustFct"].str() : "cauchy";
                int fid = -1;
                for (int i = 0; i < 8; ++i) if (fct == fcts[i]) fid = i;
                if (fid < 0) throw InvalidParameter("RobustOutlierFilter: unknown robustFct " + fct);
                const std::string sc = p["scaleEstimator"] ? p["scaleEstimator"].str() : "mad";
                int sid;
                if (sc == "none") sid = ICPMI_SCALE_NONE; else if (sc == "mad") sid = ICPMI_SCALE_MAD;
                else if (sc == "berg") sid = ICPMI_SCALE_BERG; else if (sc == "std") sid = ICPMI_SCALE_STD;
                else throw InvalidParameter("RobustOutlierFilter: unknown scaleEstimator " + sc);
                const std::string dt = p["distanceType"] ? p["distanceType"].str() : "point2point";
                int did;
                if (dt == "point2point") did = ICPMI_DIST_POINT2POINT; else if (dt == "point2plane") did = ICPMI_DIST_POINT2PLANE;
                else throw InvalidParameter("RobustOutlierFilter: unknown distanceType " + dt);
                const float apx = p["approximation"] ? p["approximation"].as<float>() : std::numeric_limits<float>::infinity();
                if (!(apx > 0.f)) throw InvalidParameter("RobustOutlierFilter: approximation must be > 0");   // (upstream's range: min 0, max inf; 0 would drop every match)
                o.type = ICPMI_OUT_ROBUST;
                o.param = p["tuning"] ? p["tuning"].as<float>() : 1.f;
                o.param2 = p["nbIterationForScale"] ? (float)p["nbIterationForScale"].as<int>() : 0.f;
                o.param3 = apx;
                o.iparam = fid | (sid << 4) | (did << 8);
            }
            else throw InvalidParameter("unknown outlier filter " + e.first);
            if (cfg.n_outlier >= 8) throw InvalidParameter("at most 8 outlier filters");
            cfg.outlier[cfg.n_outlier++] = o;
        }
    intensity = IntensityTerm{};
    if (icp["errorMinimizer"]) parseErrorMinimizer(icp["errorMinimizer"], cfg, planeEpsilon, planeModel, &intensity);
    checkVoxelChain(voxelSize, cfg.n_outlier, cfg.minimizer, planeModel);
    if (icp["transformationCheckers"].IsSequence())
        for (const auto& item : icp["transformationCheckers"].seq) {
            auto e = singleEntry(item, "transformation checker");
            if (e.first == "CounterTransformationChecker") {
                requireKnown(e.second, {"maxIterationCount"}, e.first);
                if (e.second["maxIterationCount"]) cfg.max_iterations = e.second["maxIterationCount"].as<int>();
            } else if (e.first == "DifferentialTransformationChecker") {
                requireKnown(e.second, {"minDiffRotErr", "minDiffTransErr", "smoothLength"}, e.first);
                cfg.use_differential = 1;
                if (e.second["minDiffRotErr"]) cfg.min_diff_rot = e.second["minDiffRotErr"].as<float>();
                if (e.second["minDiffTransErr"]) cfg.min_diff_trans = e.second["minDiffTransErr"].as<float>();
                if (e.second["smoothLength"]) cfg.smooth_length = e.second["smoothLength"].as<int>();
            } else if (e.first == "BoundTransformationChecker") {
                requireKnown(e.second, {"maxRotationNorm", "maxTranslationNorm"}, e.first);
                cfg.use_bound = 1;
                if (e.second["maxRotationNorm"]) cfg.max_rot_norm = e.second["maxRotationNorm"].as<float>();
                if (e.second["maxTranslationNorm"]) cfg.max_trans_norm = e.second["maxTranslationNorm"].as<float>();
            } else throw InvalidParameter("unknown transformation checker " + e.first);
        }
    recreate();
    check(h, icpmi_set_plane_epsilon(h, planeEpsilon));
    check(h, icpmi_set_plane_pair_model(h, planeModel));
    check(h, icpmi_set_intensity_weight(h, intensity.weight));
    if (voxelSizes.empty()) check(h, icpmi_set_voxel_matcher(h, voxelSize));
    else check(h, icpmi_set_voxel_schedule(h, voxelSizes.data(), (int32_t)voxelSizes.size()));
    auto chain = [&](const char* key) -> std::shared_ptr<DataPointsFilters> {
        if (!icp[key] || !icp[key].IsSequence() || icp[key].seq.empty()) return nullptr;
        return std::make_shared<DataPointsFilters>(icp[key], h);
    };
    readingDataPointsFilters = chain("readingDataPointsFilters");
    referenceDataPointsFilters = chain("referenceDataPointsFilters");
    readingStepDataPointsFilters = chain("readingStepDataPointsFilters");
    if (readingStepDataPointsFilters)
        for (const auto& f : readingStepDataPointsFilters->filters)
            if (!f->repeatable())
                throw InvalidParameter("readingStepDataPointsFilters: a filter whose result changes from call to call (RandomSampling with seed -1) "
                                       "cannot run inside the device-resident loop; give it a seed, or apply it as a readingDataPointsFilter");
}

bool GpuICPSequence::hasMap() const { return h && icpmi_has_map(h); }

bool GpuICPSequence::hasReadingFilters() const
{
    return (readingDataPointsFilters && readingDataPointsFilters->size()) || (readingStepDataPointsFilters && readingStepDataPointsFilters->size());
}

DataPoints GpuICPSequence::filteredReading(const DataPoints& reading) const
{
    DataPoints r = reading;
    if (readingDataPointsFilters) readingDataPointsFilters->apply(r);
    if (readingStepDataPointsFilters) readingStepDataPointsFilters->apply(r);
    return r;
}

bool GpuICPSequence::setMap(const DataPoints& mapIn)
{
    int32_t accepted = 0;
    if (mapIn.getNbPoints() == 0) return false; // "Ignoring attempt to setMap with an empty map"
    DataPoints filtered;
    const DataPoints* mapp = &mapIn;
    if (referenceDataPointsFilters && referenceDataPointsFilters->size()) {
        // upstream filters the CENTRED copy of the map (mean subtracted first): filters that look at coordinates
        // (BoundingBox, DistanceLimit) mean them relative to the centroid.  The original coordinates ride along as a descriptor
        // and are put back afterwards, so that the core centres the very points the caller handed in -- unless a filter moves points
        // (VoxelGrid): its output is centred centroids, which get the mean added back (the `else` below).
        bool moves = false;
        for (const auto& f : referenceDataPointsFilters->filters) moves |= f->movesFeatures();
        filtered = mapIn;
        const size_t n = filtered.getNbPoints();
        double mean[3] = {0, 0, 0};
        for (size_t i = 0; i < n; ++i) for (int r = 0; r < 3; ++r) mean[r] += filtered.col(i)[r];
        std::vector<float> orig(3 * n);
        for (size_t i = 0; i < n; ++i)
            for (int r = 0; r < 3; ++r) { orig[3 * i + r] = filtered.col(i)[r]; filtered.col(i)[r] = (float)(filtered.col(i)[r] - mean[r] / (double)n); }
        if (!moves) filtered.addDescriptor("__icpmi_original_xyz", 3, std::move(orig));
        referenceDataPointsFilters->apply(filtered);
        const size_t m = filtered.getNbPoints();
        if (filtered.descriptorExists("__icpmi_original_xyz")) {
            const Descriptor& o = filtered.getDescriptorByName("__icpmi_original_xyz");
            for (size_t i = 0; i < m; ++i) for (int r = 0; r < 3; ++r) filtered.col(i)[r] = o.data[3 * i + r];
            filtered.removeDescriptor("__icpmi_original_xyz");
        } else
            for (size_t i = 0; i < m; ++i) for (int r = 0; r < 3; ++r) filtered.col(i)[r] = (float)(filtered.col(i)[r] + mean[r] / (double)n);
        if (m == 0) return false;
        mapp = &filtered;
    }
    const DataPoints& map = *mapp;
    const float* normals = nullptr;
    if (map.descriptorExists("normals")) {
        const Descriptor& d = map.getDescriptorByName("normals");
        if (d.span != 3) throw InvalidField("descriptor normals must have 3 rows");
        normals = d.data.data();
    }
    // a point-to-plane chain against a map without `normals`: the map is accepted (upstream's setMap does not look) and the
    // registration raises InvalidField("normals"), as upstream's minimiser does
    check(h, icpmi_set_map(h, map.features.data(), (int64_t)map.getNbPoints(), normals, &accepted));
    if (accepted && !genericDescName.empty()) {
        // GenericDescriptorOutlierFilter{source: reference}: the descriptor it reads travels as the map's tracked scalar channel
        if (!map.descriptorExists(genericDescName) || map.getDescriptorByName(genericDescName).span != 1)
            throw InvalidField("GenericDescriptorOutlierFilter: the reference has no 1-row descriptor " + genericDescName);
        uploadMapScalar(map.getDescriptorByName(genericDescName).data);
    }
    if (accepted && !intensity.descName.empty()) {
        // IntensityPointToPlaneErrorMinimizer: the map's row of its descriptor, behind every index build (the device computes the gradients)
        if (!map.descriptorExists(intensity.descName) || map.getDescriptorByName(intensity.descName).span != 1)
            throw InvalidField("IntensityPointToPlaneErrorMinimizer: the reference has no 1-row descriptor " + intensity.descName);
        if (normals) check(h, icpmi_set_map_intensity(h, map.getDescriptorByName(intensity.descName).data.data(), (int64_t)map.getNbPoints(), intensity.knn));
        // (without `normals` the registration raises InvalidField("normals"), as for PointToPlaneErrorMinimizer)
    }
    return accepted != 0;
}

void GpuICPSequence::armReadingIntensity(const DataPoints& reading) const
{
    if (intensity.descName.empty()) return;
    if (!reading.descriptorExists(intensity.descName) || reading.getDescriptorByName(intensity.descName).span != 1)
        throw InvalidField("IntensityPointToPlaneErrorMinimizer: the reading has no 1-row descriptor " + intensity.descName);
    check(h, icpmi_set_reading_intensity(h, reading.getDescriptorByName(intensity.descName).data.data(), (int64_t)reading.getNbPoints()));
}

void GpuICPSequence::mapUpdatePointDistance(const DataPoints& input, float minDist, int normalsKnn, std::vector<uint8_t>& keep, int64_t& appended,
                                            int64_t& mapSize)
{
    const float* normals = nullptr;
    if (normalsKnn <= 0 && input.descriptorExists("normals") && input.getDescriptorByName("normals").span == 3)
        normals = input.getDescriptorByName("normals").data.data();
    keep.assign(input.getNbPoints(), 0);
    check(h, icpmi_map_update_point_distance(h, input.features.data(), (int64_t)input.getNbPoints(), normals, minDist, normalsKnn, keep.data(),
                                             &appended, &mapSize));
}

Mat4 GpuICPSequence::registerWithPrior(const DataPoints& scan, const Mat4& prior)
{
    Mat4 T = Mat4::identity();
    stagedPoints = scan.getNbPoints();
    haveCovariance = false; haveLocalizability = false;
    armReadingIntensity(scan); // IntensityPointToPlaneErrorMinimizer: a descriptor row does not move with the prior
    check(h, icpmi_register_prior(h, scan.features.data(), (int64_t)scan.getNbPoints(), prior.data(), T.data(), &lastStats));
    keepCovariance();
    return T;
}

SweepRegistration GpuICPSequence::registerSweep(const DataPoints& scan, const std::vector<float>& tRel, const Mat4& priorBegin, const Mat4& priorEnd,
                                                const icpmi_sweep_options& opts)
{
    if (tRel.size() != scan.getNbPoints()) throw InvalidParameter("registerSweep: one point time per point is needed");
    if (hasReadingFilters()) throw InvalidParameter("registerSweep: readingDataPointsFilters would drop points behind their times; filter the input instead");
    SweepRegistration r;
    haveCovariance = false; haveLocalizability = false; // (the matcher's buffers are reused)
    check(h, icpmi_register_sweep(h, scan.features.data(), (int64_t)scan.getNbPoints(), tRel.data(), priorBegin.data(), priorEnd.data(), &opts, &r.stats,
                                  nullptr));
    std::memcpy(r.begin.data(), r.stats.T_begin, sizeof(float) * 16);
    std::memcpy(r.end.data(), r.stats.T_end, sizeof(float) * 16);
    return r;
}

void GpuICPSequence::mapUpdateStaged(const Mat4& correction, float minDist, int normalsKnn, std::vector<uint8_t>& keep, int64_t& appended,
                                     int64_t& mapSize)
{
    keep.assign(stagedPoints, 0);
    check(h, icpmi_map_update_staged(h, correction.data(), minDist, normalsKnn, keep.data(), &appended, &mapSize));
}

static std::vector<float> scalarRow(const DataPoints& cloud, const std::string& name)
{
    const Descriptor& d = cloud.getDescriptorByName(name);
    const size_t n = cloud.getNbPoints();
    std::vector<float> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = d.data[(size_t)d.span * i];
    return out;
}

void GpuICPSequence::mapUpdateChain(const DataPoints* input, const Mat4& correction, const std::string& scalarName, const DataPoints& scanDescriptors,
                                    const Mat4& pose, const std::vector<icpmi_map_op>& ops, int nModules, std::vector<int32_t>& src,
                                    int64_t& prefix, int64_t& mapSize, bool wantSrc)
{
    const Mat4 toSensor = pose.inverse();
    const size_t n = input ? input->getNbPoints() : stagedPoints;
    std::vector<float> scalar;
    if (!scalarName.empty()) scalar = scalarRow(scanDescriptors, scalarName);
    const float* sp = scalarName.empty() ? nullptr : scalar.data();
    src.resize(wantSrc ? (size_t)residentMapSize() + (size_t)(nModules > 0 ? nModules : 1) * n + 1 : 0);
    int32_t* srcp = wantSrc ? src.data() : nullptr;
    int64_t* prefp = wantSrc ? &prefix : nullptr;
    prefix = 0;
    if (input) {
        const float* normals = nullptr;
        if (input->descriptorExists("normals") && input->getDescriptorByName("normals").span == 3) normals = input->getDescriptorByName("normals").data.data();
        check(h, icpmi_map_update_chain(h, input->features.data(), (int64_t)n, normals, sp, toSensor.data(), pose.data(), ops.data(), (int32_t)ops.size(), nModules,
                                        srcp, (int64_t)src.size(), prefp, &mapSize));
    } else
        check(h, icpmi_map_update_chain_staged(h, correction.data(), sp, toSensor.data(), pose.data(), ops.data(), (int32_t)ops.size(), nModules, srcp,
                                               (int64_t)src.size(), prefp, &mapSize));
    if (wantSrc) src.resize((size_t)mapSize);
}

void GpuICPSequence::uploadMapScalar(const std::vector<float>& scalar) { check(h, icpmi_set_map_scalar(h, scalar.data(), (int64_t)scalar.size())); }

std::vector<float> GpuICPSequence::downloadMapScalar() const
{
    std::vector<float> out((size_t)residentMapSize());
    if (!out.empty()) check(h, icpmi_get_map_scalar(h, out.data(), (int64_t)out.size()));
    return out;
}

std::vector<float> GpuICPSequence::downloadMapDensities() const
{
    std::vector<float> out((size_t)residentMapSize());
    if (!out.empty()) check(h, icpmi_get_map_densities(h, out.data(), (int64_t)out.size()));
    return out;
}

int64_t GpuICPSequence::residentMapSize() const
{
    int64_t m = 0;
    check(h, icpmi_get_map(h, nullptr, nullptr, 0, &m));
    return m;
}

bool GpuICPSequence::chainNeedsReadingNormals() const
{
    for (int f = 0; f < cfg.n_outlier; ++f)
        if (cfg.outlier[f].type == ICPMI_OUT_SURFACENORMAL) return true;
    return cfg.minimizer == ICPMI_MIN_PLANE_TO_PLANE;
}

DataPoints GpuICPSequence::downloadMap() const
{
    int64_t m = 0;
    check(h, icpmi_get_map(h, nullptr, nullptr, 0, &m));
    DataPoints out((size_t)m);
    if (m == 0) return out;
    std::vector<float> nrm(3 * (size_t)m);
    const icpmi_status s = icpmi_get_map(h, out.features.data(), nrm.data(), m, &m);
    if (s == ICPMI_ERR_MISSING_NORMALS) check(h, icpmi_get_map(h, out.features.data(), nullptr, m, &m));
    else { check(h, s); out.addDescriptor("normals", 3, std::move(nrm)); }
    return out;
}

Mat4 GpuICPSequence::operator()(const DataPoints& readingIn)
{
    Mat4 T = Mat4::identity();
    DataPoints owned;
    if (hasReadingFilters()) owned = filteredReading(readingIn);
    const DataPoints& reading = hasReadingFilters() ? owned : readingIn;
    const float* normals = nullptr;
    if (reading.descriptorExists("normals") && reading.getDescriptorByName("normals").span == 3)
        normals = reading.getDescriptorByName("normals").data.data();
    // ErrorMinimizer::getOverlap() (Mapper.cpp:219): a reading that carries `simpleSensorNoise` (and normals) gets upstream's
    // sensor-noise count instead of the weighted ratio; the row rides to the device ahead of the registration (one shot)
    if (!genericReadDescName.empty()) { // GenericDescriptorOutlierFilter{source: reading}
        if (!reading.descriptorExists(genericReadDescName) || reading.getDescriptorByName(genericReadDescName).span != 1)
            throw InvalidField("GenericDescriptorOutlierFilter: the reading has no 1-row descriptor " + genericReadDescName);
        check(h, icpmi_set_reading_scalar(h, reading.getDescriptorByName(genericReadDescName).data.data(), (int64_t)reading.getNbPoints()));
    }
    if (!maxDistFieldName.empty()) { // KDTreeVarDistMatcher: the radii of the FILTERED reading, ahead of the registration (one shot)
        if (!reading.descriptorExists(maxDistFieldName) || reading.getDescriptorByName(maxDistFieldName).span != 1)
            throw InvalidField("KDTreeVarDistMatcher: the reading has no 1-row descriptor " + maxDistFieldName);
        check(h, icpmi_set_reading_max_dist(h, reading.getDescriptorByName(maxDistFieldName).data.data(), (int64_t)reading.getNbPoints()));
    }
    armReadingIntensity(reading); // IntensityPointToPlaneErrorMinimizer
    // (PointToPointErrorMinimizer::getOverlap() needs the noise row alone, only PointToPlane also the reading's normals)
    if ((normals || cfg.minimizer == ICPMI_MIN_POINT_TO_POINT) && reading.descriptorExists("simpleSensorNoise") &&
        reading.getDescriptorByName("simpleSensorNoise").span == 1)
        check(h, icpmi_set_reading_sensor_noise(h, reading.getDescriptorByName("simpleSensorNoise").data.data(), (int64_t)reading.getNbPoints()));
    haveCovariance = false; haveLocalizability = false;
    check(h, icpmi_register(h, reading.features.data(), (int64_t)reading.getNbPoints(), normals, T.data(), &lastStats));
    keepCovariance();
    return T;
}

icpmi_residual GpuICPSequence::residual(const DataPoints& readingIn, const Mat4& T, int kind) const
{
    DataPoints owned;
    if (hasReadingFilters()) owned = filteredReading(readingIn);
    const DataPoints& reading = hasReadingFilters() ? owned : readingIn;
    const float* normals = nullptr;
    if (reading.descriptorExists("normals") && reading.getDescriptorByName("normals").span == 3)
        normals = reading.getDescriptorByName("normals").data.data();
    if (!genericReadDescName.empty()) { // GenericDescriptorOutlierFilter{source: reading}
        if (!reading.descriptorExists(genericReadDescName) || reading.getDescriptorByName(genericReadDescName).span != 1)
            throw InvalidField("GenericDescriptorOutlierFilter: the reading has no 1-row descriptor " + genericReadDescName);
        check(h, icpmi_set_reading_scalar(h, reading.getDescriptorByName(genericReadDescName).data.data(), (int64_t)reading.getNbPoints()));
    }
    if (!maxDistFieldName.empty()) { // KDTreeVarDistMatcher: the radii of the FILTERED reading (one shot)
        if (!reading.descriptorExists(maxDistFieldName) || reading.getDescriptorByName(maxDistFieldName).span != 1)
            throw InvalidField("KDTreeVarDistMatcher: the reading has no 1-row descriptor " + maxDistFieldName);
        check(h, icpmi_set_reading_max_dist(h, reading.getDescriptorByName(maxDistFieldName).data.data(), (int64_t)reading.getNbPoints()));
    }
    icpmi_residual out{};
    check(h, icpmi_residual_error(h, reading.features.data(), (int64_t)reading.getNbPoints(), normals, T.data(), kind, &out));
    return out;
}

icpmi_residual GpuICPSequence::residualStaged(const Mat4& T, int kind) const
{
    icpmi_residual out{};
    check(h, icpmi_residual_error_staged(h, T.data(), kind, &out));
    return out;
}

// ---- relocalisation ----------------------------------------------------------------------------
std::vector<int> rankCandidates(const PoseScores& scores, size_t n, float minPairsRatio)
{
    const double need = (double)minPairsRatio * (double)n;
    std::vector<std::pair<double, int>> keyed;
    for (size_t i = 0; i < scores.size(); ++i) {
        const icpmi_residual& r = scores.residual[i];
        if (scores.status[i] != ICPMI_OK || r.pairs <= 0 || (double)r.pairs < need) continue;
        keyed.emplace_back(r.sum_abs / (double)r.pairs, (int)i);
    }
    std::sort(keyed.begin(), keyed.end()); // (the index breaks ties)
    std::vector<int> order;
    for (const auto& kv : keyed) order.push_back(kv.second);
    return order;
}

std::vector<Mat4> candidateGrid(const Mat4& centre, float halfX, float halfY, float halfYaw, int stepsX, int stepsY, int stepsYaw)
{
    if (stepsX < 0 || stepsY < 0 || stepsYaw < 0) throw InvalidParameter("candidateGrid: steps must be >= 0");
    auto off = [](float half, int k, int steps) { return steps == 0 ? 0.0 : (double)half * (double)k / (double)steps; };
    std::vector<Mat4> out;
    out.push_back(centre);
    for (int ia = -stepsYaw; ia <= stepsYaw; ++ia) {
        const double a = off(halfYaw, ia, stepsYaw);
        const double ca = std::cos(a), sa = std::sin(a);
        const double Rz[3][3] = {{ca, -sa, 0.0}, {sa, ca, 0.0}, {0.0, 0.0, 1.0}};
        for (int iy = -stepsY; iy <= stepsY; ++iy)
            for (int ix = -stepsX; ix <= stepsX; ++ix) {
                if (ia == 0 && iy == 0 && ix == 0) continue;
                Mat4 c = centre;
                for (int r = 0; r < 3; ++r)
                    for (int col = 0; col < 3; ++col)
                        c(r, col) = (float)((Rz[r][0] * (double)centre(0, col) + Rz[r][1] * (double)centre(1, col)) + Rz[r][2] * (double)centre(2, col));
                c(0, 3) = (float)((double)centre(0, 3) + off(halfX, ix, stepsX));
                c(1, 3) = (float)((double)centre(1, 3) + off(halfY, iy, stepsY));
                out.push_back(c);
            }
    }
    return out;
}

PoseScores GpuICPSequence::residualsFiltered(const DataPoints& reading, const std::vector<Mat4>& poses, int kind) const
{
    const float* normals = nullptr;
    if (reading.descriptorExists("normals") && reading.getDescriptorByName("normals").span == 3)
        normals = reading.getDescriptorByName("normals").data.data();
    if (!genericReadDescName.empty()) { // GenericDescriptorOutlierFilter{source: reading}: one row for all poses
        if (!reading.descriptorExists(genericReadDescName) || reading.getDescriptorByName(genericReadDescName).span != 1)
            throw InvalidField("GenericDescriptorOutlierFilter: the reading has no 1-row descriptor " + genericReadDescName);
        check(h, icpmi_set_reading_scalar(h, reading.getDescriptorByName(genericReadDescName).data.data(), (int64_t)reading.getNbPoints()));
    }
    if (!maxDistFieldName.empty()) { // KDTreeVarDistMatcher: the radii of the FILTERED reading (one shot, for all poses)
        if (!reading.descriptorExists(maxDistFieldName) || reading.getDescriptorByName(maxDistFieldName).span != 1)
            throw InvalidField("KDTreeVarDistMatcher: the reading has no 1-row descriptor " + maxDistFieldName);
        check(h, icpmi_set_reading_max_dist(h, reading.getDescriptorByName(maxDistFieldName).data.data(), (int64_t)reading.getNbPoints()));
    }
    PoseScores out;
    out.residual.assign(poses.size(), icpmi_residual{});
    out.status.assign(poses.size(), ICPMI_OK);
    std::vector<float> T(16 * poses.size());
    for (size_t p = 0; p < poses.size(); ++p) std::copy(poses[p].m.begin(), poses[p].m.end(), T.begin() + 16 * p);
    int32_t batched = 0;
    check(h, icpmi_residual_error_poses(h, reading.features.data(), (int64_t)reading.getNbPoints(), normals, T.data(), (int32_t)poses.size(), kind,
                                        out.residual.data(), out.status.data(), &batched));
    out.batched = batched;
    return out;
}

PoseScores GpuICPSequence::residuals(const DataPoints& readingIn, const std::vector<Mat4>& poses, int kind) const
{
    if (!hasReadingFilters()) return residualsFiltered(readingIn, poses, kind);
    return residualsFiltered(filteredReading(readingIn), poses, kind);
}

// icpmi_register_multistart carries the points alone, as icpmi_register_prior does: a chain that reads the reading's normals or one of its
// descriptor rows cannot go through it (Mapper::processInput keeps such chains off the prior path for the same reason)
void GpuICPSequence::requireBareReadingChain(const char* who) const
{
    if (chainNeedsReadingNormals())
        throw InvalidParameter(std::string(who) + ": the chain (SurfaceNormalOutlierFilter, PlaneToPlaneErrorMinimizer, SymmetricPointToPlaneErrorMinimizer) reads the reading's normals, which the multistart registration does not carry");
    if (readsReadingDescriptor())
        throw InvalidParameter(std::string(who) + ": the chain reads a descriptor row of the reading (" +
                               (!genericReadDescName.empty() ? genericReadDescName : !maxDistFieldName.empty() ? maxDistFieldName : intensity.descName) + "), which the multistart registration does not carry");
}

MultiStartResult GpuICPSequence::multiStartFiltered(const DataPoints& reading, const std::vector<Mat4>& priors)
{
    requireBareReadingChain("registerMultiStart");
    MultiStartResult out;
    out.correction.assign(priors.size(), Mat4::identity());
    out.stats.assign(priors.size(), icpmi_stats{});
    out.status.assign(priors.size(), ICPMI_OK);
    std::vector<float> P(16 * priors.size()), T(16 * priors.size());
    for (size_t s = 0; s < priors.size(); ++s) std::copy(priors[s].m.begin(), priors[s].m.end(), P.begin() + 16 * s);
    stagedPoints = 0;
    haveCovariance = false; haveLocalizability = false;
    check(h, icpmi_register_multistart(h, reading.features.data(), (int64_t)reading.getNbPoints(), P.data(), (int32_t)priors.size(), 0, T.data(),
                                       out.stats.data(), out.status.data()));
    for (size_t s = 0; s < priors.size(); ++s) std::copy(T.begin() + 16 * s, T.begin() + 16 * s + 16, out.correction[s].m.begin());
    return out;
}

MultiStartResult GpuICPSequence::registerMultiStart(const DataPoints& readingIn, const std::vector<Mat4>& priors)
{
    if (!hasReadingFilters()) return multiStartFiltered(readingIn, priors);
    return multiStartFiltered(filteredReading(readingIn), priors);
}

Relocalization GpuICPSequence::relocalize(const DataPoints& readingIn, const std::vector<Mat4>& candidates, const RelocalizeOptions& options)
{
    if (candidates.empty()) throw InvalidParameter("relocalize: no candidates");
    requireBareReadingChain("relocalize"); // (before anything is scored: the refinement could not run)
    DataPoints owned;
    if (hasReadingFilters()) owned = filteredReading(readingIn); // once for the three passes
    const DataPoints& reading = hasReadingFilters() ? owned : readingIn;
    const size_t n = reading.getNbPoints();
    Relocalization out;
    out.scores = residualsFiltered(reading, candidates, options.kind);
    const std::vector<int> order = rankCandidates(out.scores, n, options.minPairsRatio);
    if (order.empty()) throw ConvergenceError("relocalize: no candidate survived the scoring");
    const size_t k = std::min<size_t>(order.size(), (size_t)std::max(1, std::min(options.refine, 16)));
    std::vector<Mat4> best(k), refined(k);
    for (size_t i = 0; i < k; ++i) best[i] = candidates[(size_t)order[i]];
    const MultiStartResult ms = multiStartFiltered(reading, best);
    for (size_t i = 0; i < k; ++i) refined[i] = ms.correction[i] * best[i];
    PoseScores again = residualsFiltered(reading, refined, options.kind);
    for (size_t i = 0; i < k; ++i) if (ms.status[i] != ICPMI_OK) again.status[i] = ms.status[i]; // a start that did not converge is out
    const std::vector<int> fin = rankCandidates(again, n, options.minPairsRatio);
    if (fin.empty()) throw ConvergenceError("relocalize: no refined candidate survived the scoring");
    const size_t w = (size_t)fin[0];
    out.pose = refined[w];
    out.residual = again.residual[w];
    out.index = order[w];
    return out;
}

// ---- relocalisation on the voxel path -----------------------------------------------------------
std::vector<int> rankVoxelCandidates(const VoxelPoseScores& scores, size_t n, float minPairsRatio)
{
    const double need = (double)minPairsRatio * (double)n;
    std::vector<std::pair<double, int>> keyed;
    for (size_t i = 0; i < scores.size(); ++i) {
        const icpmi_voxel_score& r = scores.score[i];
        if (scores.status[i] != ICPMI_OK || r.pairs <= 0 || (double)r.pairs < need) continue;
        keyed.emplace_back(-(r.likelihood / (double)n), (int)i);
    }
    std::sort(keyed.begin(), keyed.end()); // (the index breaks ties)
    std::vector<int> order;
    for (const auto& kv : keyed) order.push_back(kv.second);
    return order;
}

VoxelPoseScores GpuICPSequence::voxelScoresFiltered(const DataPoints& reading, const std::vector<Mat4>& poses, int level, float beta) const
{
    const float* normals = nullptr;
    if (reading.descriptorExists("normals") && reading.getDescriptorByName("normals").span == 3)
        normals = reading.getDescriptorByName("normals").data.data();
    VoxelPoseScores out;
    out.score.assign(poses.size(), icpmi_voxel_score{});
    out.status.assign(poses.size(), ICPMI_OK);
    std::vector<float> T(16 * poses.size());
    for (size_t p = 0; p < poses.size(); ++p) std::copy(poses[p].m.begin(), poses[p].m.end(), T.begin() + 16 * p);
    icpmi_voxel_score_options opt;
    icpmi_voxel_score_options_default(&opt);
    opt.level = level; opt.beta = beta;
    check(h, icpmi_voxel_score_poses(h, reading.features.data(), (int64_t)reading.getNbPoints(), normals, T.data(), (int32_t)poses.size(), &opt,
                                     out.score.data(), out.status.data()));
    return out;
}

VoxelPoseScores GpuICPSequence::voxelScores(const DataPoints& readingIn, const std::vector<Mat4>& poses, int level, float beta) const
{
    if (!hasReadingFilters()) return voxelScoresFiltered(readingIn, poses, level, beta);
    return voxelScoresFiltered(filteredReading(readingIn), poses, level, beta);
}

// ---- global localisation (include/icpmi.h: icpmi_global_localize) -----------------
std::vector<Rot9> yawRotations(int steps, double roll, double pitch)
{
    if (steps < 1) throw InvalidParameter("yawRotations: steps must be >= 1");
    const double cr = std::cos(roll), sr = std::sin(roll), cp = std::cos(pitch), sp = std::sin(pitch);
    const double Rx[3][3] = {{1.0, 0.0, 0.0}, {0.0, cr, -sr}, {0.0, sr, cr}};
    const double Ry[3][3] = {{cp, 0.0, sp}, {0.0, 1.0, 0.0}, {-sp, 0.0, cp}};
    double Ryx[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ryx[r][c] = (Ry[r][0] * Rx[0][c] + Ry[r][1] * Rx[1][c]) + Ry[r][2] * Rx[2][c];
    std::vector<Rot9> out((size_t)steps);
    for (int i = 0; i < steps; ++i) {
        const double a = 2.0 * M_PI * (double)i / (double)steps;
        const double ca = std::cos(a), sa = std::sin(a);
        const double Rz[3][3] = {{ca, -sa, 0.0}, {sa, ca, 0.0}, {0.0, 0.0, 1.0}};
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) out[(size_t)i][(size_t)(3 * c + r)] = (float)((Rz[r][0] * Ryx[0][c] + Rz[r][1] * Ryx[1][c]) + Rz[r][2] * Ryx[2][c]);
    }
    return out;
}

icpmi_global_localize_result GpuICPSequence::globalLocalize(const DataPoints& readingIn, const std::vector<Rot9>& rotations,
                                                            const GlobalLocalizeOptions& options) const
{
    DataPoints owned;
    if (hasReadingFilters()) owned = filteredReading(readingIn);
    const DataPoints& reading = hasReadingFilters() ? owned : readingIn;
    icpmi_global_localize_options opt;
    icpmi_global_localize_options_default(&opt);
    opt.cell_size = options.cellSize; opt.levels = options.levels; opt.min_score_ratio = options.minScoreRatio;
    opt.max_nodes = options.maxNodes; opt.batch = options.batch; opt.has_box = options.hasBox ? 1 : 0;
    for (int j = 0; j < 3; ++j) { opt.box_lo[j] = options.boxLo[(size_t)j]; opt.box_hi[j] = options.boxHi[(size_t)j]; }
    icpmi_global_localize_result res{};
    check(h, icpmi_global_localize(h, reading.features.data(), (int64_t)reading.getNbPoints(), rotations.empty() ? nullptr : rotations[0].data(),
                                   (int32_t)rotations.size(), &opt, &res));
    return res;
}

GlobalRelocalization GpuICPSequence::relocalizeGlobal(const DataPoints& reading, const std::vector<Rot9>& rotations, const GlobalLocalizeOptions& options,
                                                      const RelocalizeOptions& refine, const RelocalizeVoxelOptions& refineVoxel)
{
    GlobalRelocalization out;
    out.search = globalLocalize(reading, rotations, options);
    if (!out.search.found) throw ConvergenceError("relocalizeGlobal: no pose reaches minScoreRatio");
    Mat4 start;
    std::copy(out.search.T, out.search.T + 16, start.m.begin());
    out.voxel = voxelSize > 0.f;
    if (out.voxel) { out.refinedVoxel = relocalizeVoxel(reading, {start}, refineVoxel); out.pose = out.refinedVoxel.pose; }
    else { out.refined = relocalize(reading, {start}, refine); out.pose = out.refined.pose; }
    return out;
}

// ---- many readings, or many starts, in one loop on the voxel path (include/icpmi.h: icpmi_voxel_register_*) ----
static const float* normalsOf(const DataPoints& cloud)
{
    if (cloud.descriptorExists("normals") && cloud.getDescriptorByName("normals").span == 3) return cloud.getDescriptorByName("normals").data.data();
    return nullptr;
}

MultiStartResult GpuICPSequence::registerVoxelBatch(const std::vector<DataPoints>& readingsIn)
{
    const size_t B = readingsIn.size();
    std::vector<DataPoints> owned;
    if (hasReadingFilters()) for (const DataPoints& r : readingsIn) owned.push_back(filteredReading(r)); // once per reading
    const std::vector<DataPoints>& readings = hasReadingFilters() ? owned : readingsIn;
    MultiStartResult out;
    out.correction.assign(B, Mat4::identity());
    out.stats.assign(B, icpmi_stats{});
    out.status.assign(B, ICPMI_OK);
    std::vector<const float*> pts(B), nrm(B);
    std::vector<int64_t> ns(B);
    for (size_t b = 0; b < B; ++b) { pts[b] = readings[b].features.data(); nrm[b] = normalsOf(readings[b]); ns[b] = (int64_t)readings[b].getNbPoints(); }
    std::vector<float> T(16 * std::max<size_t>(B, 1));
    stagedPoints = 0;
    haveCovariance = false; haveLocalizability = false;
    check(h, icpmi_voxel_register_batch(h, (int32_t)B, pts.data(), ns.data(), nrm.data(), 0, T.data(), out.stats.data(), out.status.data()));
    for (size_t b = 0; b < B; ++b) std::copy(T.begin() + 16 * b, T.begin() + 16 * b + 16, out.correction[b].m.begin());
    if (B) lastStats = out.stats.back();
    return out;
}

MultiStartResult GpuICPSequence::voxelMultiStartFiltered(const DataPoints& reading, const std::vector<Mat4>& priors)
{
    const size_t S = priors.size();
    MultiStartResult out;
    out.correction.assign(S, Mat4::identity());
    out.stats.assign(S, icpmi_stats{});
    out.status.assign(S, ICPMI_OK);
    std::vector<float> P(16 * std::max<size_t>(S, 1)), T(16 * std::max<size_t>(S, 1));
    for (size_t s = 0; s < S; ++s) std::copy(priors[s].m.begin(), priors[s].m.end(), P.begin() + 16 * s);
    stagedPoints = 0;
    haveCovariance = false; haveLocalizability = false;
    check(h, icpmi_voxel_register_multistart(h, reading.features.data(), (int64_t)reading.getNbPoints(), normalsOf(reading), P.data(), (int32_t)S, 0,
                                             T.data(), out.stats.data(), out.status.data()));
    for (size_t s = 0; s < S; ++s) std::copy(T.begin() + 16 * s, T.begin() + 16 * s + 16, out.correction[s].m.begin());
    if (S) lastStats = out.stats.back();
    return out;
}

MultiStartResult GpuICPSequence::registerVoxelMultiStart(const DataPoints& readingIn, const std::vector<Mat4>& priors)
{
    if (!hasReadingFilters()) return voxelMultiStartFiltered(readingIn, priors);
    return voxelMultiStartFiltered(filteredReading(readingIn), priors);
}

// icpmi_get_voxel_batch_report: one entry per level the member entered
std::vector<GpuICPSequence::VoxelLevelReport> GpuICPSequence::voxelBatchReport(int member) const
{
    int32_t levels = 0, it[4], pf[4], pl[4];
    check(h, icpmi_get_voxel_batch_report(h, member, &levels, it, pf, pl));
    std::vector<VoxelLevelReport> out;
    for (int l = 0; l < levels && l < 4; ++l) out.push_back({it[l], pf[l], pl[l]});
    return out;
}

VoxelRelocalization GpuICPSequence::relocalizeVoxel(const DataPoints& readingIn, const std::vector<Mat4>& candidates, const RelocalizeVoxelOptions& options)
{
    if (candidates.empty()) throw InvalidParameter("relocalizeVoxel: no candidates");
    DataPoints owned;
    if (hasReadingFilters()) owned = filteredReading(readingIn); // once for the three passes
    const DataPoints& reading = hasReadingFilters() ? owned : readingIn;
    const size_t n = reading.getNbPoints();
    VoxelRelocalization out;
    out.scores = voxelScoresFiltered(reading, candidates, options.level, options.beta);
    const std::vector<int> order = rankVoxelCandidates(out.scores, n, options.minPairsRatio);
    if (order.empty()) throw ConvergenceError("relocalizeVoxel: no candidate survived the scoring");
    const size_t k = std::min<size_t>(order.size(), (size_t)std::max(1, options.refine));
    std::vector<Mat4> refined(k);
    std::vector<icpmi_status> status(k, ICPMI_OK);
    // the chain as it is, the whole schedule, the starts of a chunk of 16 in one loop: every start is bit for bit the reading moved by its
    // candidate and registered alone (a voxel chain reads no row of the reading but its normals)
    for (size_t c0 = 0; c0 < k; c0 += 16) {
        const size_t cn = std::min<size_t>(16, k - c0);
        std::vector<Mat4> chunk(cn);
        for (size_t j = 0; j < cn; ++j) chunk[j] = candidates[(size_t)order[c0 + j]];
        const MultiStartResult ms = voxelMultiStartFiltered(reading, chunk);
        for (size_t j = 0; j < cn; ++j) {
            const icpmi_status s = ms.status[j];
            if (s == ICPMI_ERR_NO_POINT_TO_MINIMIZE || s == ICPMI_ERR_NO_OUTLIER_TO_FILTER || s == ICPMI_ERR_BOUND || s == ICPMI_ERR_NAN) {
                status[c0 + j] = s; refined[c0 + j] = chunk[j]; // a start that did not converge is out
                continue;
            }
            check(h, s);
            refined[c0 + j] = ms.correction[j] * chunk[j];
        }
    }
    VoxelPoseScores again = voxelScoresFiltered(reading, refined, -1, options.beta);
    for (size_t i = 0; i < k; ++i) if (status[i] != ICPMI_OK) again.status[i] = status[i];
    const std::vector<int> fin = rankVoxelCandidates(again, n, options.minPairsRatio);
    if (fin.empty()) throw ConvergenceError("relocalizeVoxel: no refined candidate survived the scoring");
    const size_t w = (size_t)fin[0];
    out.pose = refined[w];
    out.score = again.score[w];
    out.index = order[w];
    return out;
}

float GpuICPSequence::ErrorMinimizerView::getResidualError(const DataPoints& reading, const Mat4& T) const
{
    return (float)owner->residual(reading, T).sum_abs;
}

// ------------------------------------------------------------------------------------------------
DataPoints RigidTransformation::compute(const DataPoints& cloud, const Mat4& T) const
{
    DataPoints out = cloud;
    const int64_t n = (int64_t)cloud.getNbPoints();
    const int dn = cloud.findDescriptor("normals");
    const float* nin = dn >= 0 && cloud.descriptors[dn].span == 3 ? cloud.descriptors[dn].data.data() : nullptr;
    float* nout = nin ? out.descriptors[dn].data.data() : nullptr;
    icpmi_status s = icpmi_transform(h, T.data(), cloud.features.data(), n, out.features.data(), nin, nout);
    if (s == ICPMI_ERR_INVALID_ARG) throw TransformationError(icpmi_last_error(h));
    GpuICPSequence::check(h, s);
    const int dobs = cloud.findDescriptor("observationDirections");
    if (dobs >= 0 && cloud.descriptors[dobs].span == 3 && n > 0) {
        // rotate the second direction field with the same operator (features are recomputed, cheap)
        std::vector<float> scratch(cloud.features.size());
        GpuICPSequence::check(h, icpmi_transform(h, T.data(), cloud.features.data(), n, scratch.data(),
                                                 cloud.descriptors[dobs].data.data(), out.descriptors[dobs].data.data()));
    }
    return out;
}

// the DataPointsFilter classes and their factory: DataPointsFilters.cpp

} // namespace nim
