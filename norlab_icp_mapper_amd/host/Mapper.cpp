// Mapper.cpp -- see Mapper.h.
#include "Mapper.h"
#include <thread>

#include <algorithm>
#include <cmath>
#include <iterator>
#include <fstream>
#include <iostream>
#include <sstream>
#include <unordered_set>

namespace nim {

void Trajectory::save(const std::string& filename) const
{
    // positions as features, rotation columns as orientationX/Y/Z, stamps as the int64 time row "t" holding
    // `time_since_epoch().count()` (Trajectory.cpp:15-53: DataPoints(features, labels, descriptors, labels, times, timeLabels))
    const size_t n = poses.size();
    DataPoints cloud(n);
    std::vector<float> ox(3 * n), oy(3 * n), oz(3 * n);
    std::vector<std::int64_t> t(n);
    for (size_t i = 0; i < n; ++i) {
        for (int r = 0; r < 3; ++r) {
            cloud.col(i)[r] = poses[i](r, 3);
            ox[3 * i + r] = poses[i](r, 0); oy[3 * i + r] = poses[i](r, 1); oz[3 * i + r] = poses[i](r, 2);
        }
        t[i] = (std::int64_t)stamps[i].time_since_epoch().count();
    }
    cloud.addDescriptor("orientationX", 3, std::move(ox));
    cloud.addDescriptor("orientationY", 3, std::move(oy));
    if (dimension == 3) cloud.addDescriptor("orientationZ", 3, std::move(oz));
    cloud.addTime("t", 1, std::move(t));
    cloud.save(filename);
}

void Mapper::fillRegistrar()
{
    registrar.add("PointDistanceMapperModule", [](const yaml::Node& p, icpmi_handle h) { return std::make_shared<PointDistanceMapperModule>(p, h); });
    registrar.add("OctreeMapperModule", [](const yaml::Node& p, icpmi_handle h) { return std::make_shared<OctreeMapperModule>(p, h); });
    registrar.add("DynamicPointsMapperModule", [](const yaml::Node& p, icpmi_handle h) { return std::make_shared<DynamicPointsMapperModule>(p, h); });
}

Mapper::Mapper(const std::string& configFilePath, bool is3D_, bool isOnline_, bool isMapping_, bool saveMapCellsOnHardDrive, int device)
    : icp(device), is3D(is3D_), isOnline(isOnline_), isMapping(isMapping_),
      map(is3D_, isOnline_, saveMapCellsOnHardDrive, icp, icpMapLock), trajectory(is3D_ ? 3 : 2), transformation(icp.handle())
{
    fillRegistrar();
    loadYamlConfig(configFilePath);
    rebuildRadiusFilter();
}

Mapper::~Mapper()
{
    if (mapUpdateFuture.valid()) mapUpdateFuture.wait();
}

void Mapper::rebuildRadiusFilter()
{
    // DistanceLimitDataPointsFilter{dim: -1, dist: sensorMaxRange, removeInside: 0} (Mapper.cpp:27-31)
    std::ostringstream y;
    y << "{dim: -1, dist: " << map.getSensorMaxRange() << ", removeInside: 0}";
    radiusFilter = createDataPointsFilter("DistanceLimitDataPointsFilter", yaml::Load(y.str()), icp.handle());
}

namespace {

// every key must be one of `allowed`, at most once (the reference's validateYamlKeys messages)
void requireOnlyKeys(const yaml::Node& node, std::initializer_list<const char*> allowed)
{
    if (!node.IsMap()) throw yaml::Exception("Expected a YAML Map node.");
    std::unordered_set<std::string> seen;
    for (const auto& entry : node.map) {
        const std::string& key = entry.first;
        if (!seen.insert(key).second) throw yaml::Exception("Duplicated key: " + key);
        const bool known = std::any_of(allowed.begin(), allowed.end(), [&](const char* a) { return key == a; });
        if (!known) throw yaml::Exception("Invalid key: " + key);
    }
}

std::string slurp(const std::string& path)
{
    std::ifstream in(path.c_str());
    if (!in) throw std::runtime_error("The input config file " + path + " does not exist");
    return std::string(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

} // namespace

UpdatePolicy UpdatePolicy::fromYaml(const yaml::Node& uc)
{
    requireOnlyKeys(uc, {"type", "value"});
    for (const char* k : {"type", "value"})
        if (!uc[k]) throw yaml::Exception(std::string("Missing key: ") + k);
    // one row per condition: name, tag, admissible range of the value
    struct Row { const char* name; Kind kind; float lo, hi; };
    static const Row rows[] = {
        {"distance", Distance, 0.f, INFINITY},
        {"overlap", Overlap, 0.f, 1.f},
        {"delay", Delay, 0.f, INFINITY},
    };
    const std::string type = uc["type"].as<std::string>();
    const float value = uc["value"].as<float>();
    for (const Row& r : rows) {
        if (type != r.name) continue;
        if (!(value >= r.lo && value <= r.hi)) throw yaml::Exception("Invalid map update " + type + ": " + std::to_string(value));
        UpdatePolicy p; p.kind = r.kind; p.threshold = value;
        return p;
    }
    throw yaml::Exception("Invalid map update condition: " + type);
}

void Mapper::loadYamlConfig(const std::string& configFilePath) { loadYamlConfigFromString(slurp(configFilePath)); }

void Mapper::loadYamlConfigFromString(const std::string& text)
{
    const yaml::Node root = yaml::Load(text);
    requireOnlyKeys(root, {"icp", "input", "post", "mapper"});
    const auto announceMissing = [](const char* what) { std::cout << what << std::endl; };

    // 1. the registration chain; loadFromYamlNode / setDefault re-create the GPU-side chain, so nobody may be using it
    {
        std::lock_guard<std::mutex> g(icpMapLock);
        if (const yaml::Node& chain = root["icp"]) icp.loadFromYamlNode(chain);
        else { announceMissing("icp config not found, using default"); icp.setDefault(); }
    }
    // 2. everything that shares the GPU context of that chain
    transformation = RigidTransformation(icp.handle());
    struct FilterSection { const char* key; DataPointsFilters* target; const char* missing; };
    const FilterSection sections[] = {
        {"input", &inputFilters, "Input config not found, using empty configuration."},
        {"post", &mapPostFilters, "Post config not found, using empty configuration."},
    };
    for (const FilterSection& sec : sections) {
        if (const yaml::Node& n = root[sec.key]) *sec.target = DataPointsFilters(n, icp.handle());
        else announceMissing(sec.missing);
    }
    // 3. map growth
    if (!root["mapper"]) announceMissing("mapper config not found, using default");
    configureMapperSection(root["mapper"]);
}

void Mapper::configureMapperSection(const yaml::Node& mapperNode)
{
    const bool present = (bool)mapperNode;
    if (present && mapperNode["updateCondition"]) updatePolicy = UpdatePolicy::fromYaml(mapperNode["updateCondition"]);
    else {
        if (present) std::cout << "Mapper update condition not found, using default configuration." << std::endl;
        updatePolicy = UpdatePolicy(); // distance, 1 m
    }
    if (present && mapperNode["sensorMaxRange"]) {
        const float range = mapperNode["sensorMaxRange"].as<float>();
        if (range < 0) throw yaml::Exception("Invalid sensor max range: " + std::to_string(range));
        map.setSensorMaxRange(range);
    }
    if (present && mapperNode["mapperModule"]) {
        const yaml::Node& modules = mapperNode["mapperModule"];
        if (!modules.IsSequence()) throw yaml::Exception("mapperModule must be a sequence");
        for (const auto& item : modules.seq) map.addMapperModule(registrar.createFromYAML(item, icp.handle()));
    } else {
        if (present) std::cout << "mapper module not found, using default" << std::endl;
        setDefaultMapperModule();
    }
}

void Mapper::setDefaultMapperModule()
{
    // PointDistanceMapperModule{minDistNewPoint: 0.15} (Mapper.cpp:330-336)
    map.addMapperModule(registrar.create("PointDistanceMapperModule", yaml::Load("{minDistNewPoint: 0.15}"), icp.handle()));
}

// the points' times as offsets from the stamp: the float descriptor, or else the int64 row of absolute nanoseconds; returns seconds per unit
static double sweepPointTimes(const DataPoints& cloud, int64_t stampNs, const std::string& timeField, double timeUnit, const char* who, std::vector<float>& tRel)
{
    const size_t n = cloud.getNbPoints();
    if (cloud.descriptorExists(timeField)) {
        const Descriptor& d = cloud.getDescriptorByName(timeField);
        if (d.span != 1) throw InvalidField(std::string(who) + ": descriptor " + timeField + " must have one row");
        tRel = d.data;
        return timeUnit;
    }
    if (cloud.timeExists(timeField)) {
        const TimeField& t = cloud.getTimeByName(timeField);
        if (t.span != 1) throw InvalidField(std::string(who) + ": time " + timeField + " must have one row");
        tRel.resize(n);
        for (size_t i = 0; i < n; ++i) tRel[i] = (float)(t.data[i] - stampNs);
        return 1e-9;
    }
    throw InvalidField(std::string(who) + ": the cloud has neither a descriptor nor a time row called " + timeField);
}

void deskewSweep(icpmi_handle ctx, DataPoints& cloud, const SweepMotion& motion, TimePoint stamp, const DeskewOptions& opts)
{
    const size_t n = cloud.getNbPoints();
    const int64_t stampNs = (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(stamp.time_since_epoch()).count();
    std::vector<float> tRel;
    const double unit = sweepPointTimes(cloud, stampNs, opts.timeField, opts.timeUnit, "deskew", tRel);
    if (motion.stampNs.size() != motion.pose.size()) throw InvalidParameter("deskew: the motion has " + std::to_string(motion.stampNs.size()) +
                                                                            " stamps for " + std::to_string(motion.pose.size()) + " poses");
    // the sign-continued table is built from this once per call: one call per scan (a second one for observationDirections)
    std::vector<double> stampS(motion.stampNs.size()), pose7(7 * motion.pose.size());
    for (size_t k = 0; k < stampS.size(); ++k) {
        stampS[k] = 1e-9 * (double)(motion.stampNs[k] - stampNs);
        std::copy(motion.pose[k].begin(), motion.pose[k].end(), pose7.begin() + 7 * k);
    }
    icpmi_sweep_motion m{};
    m.n_poses = (int32_t)std::min<size_t>(stampS.size(), (size_t)ICPMI_DESKEW_MAX_POSES + 1);
    m.extrapolate = opts.extrapolate ? 1 : 0;
    m.stamp_s = stampS.data(); m.pose7 = pose7.data();
    m.ref_s = opts.refS; m.time_unit_s = unit; m.round_s = 1e-9 * (double)opts.roundToNs;
    std::vector<float> out(4 * n);
    const bool hasNormals = cloud.descriptorExists("normals"), hasObs = cloud.descriptorExists("observationDirections");
    for (const char* name : {"normals", "observationDirections"})
        if (cloud.descriptorExists(name) && cloud.getDescriptorByName(name).span != 3) throw InvalidField(std::string("deskew: descriptor ") + name + " must have three rows");
    std::vector<float> rotated;
    if (hasNormals || !hasObs) {
        float* nrm = hasNormals ? cloud.getDescriptorByName("normals").data.data() : nullptr;
        if (hasNormals) rotated.resize(3 * n);
        GpuICPSequence::check(ctx, icpmi_deskew(ctx, cloud.features.data(), (int64_t)n, tRel.data(), &m, out.data(), nrm, hasNormals ? rotated.data() : nullptr));
        if (hasNormals) cloud.getDescriptorByName("normals").data.swap(rotated);
    }
    if (hasObs) { // the same pass with that row in the normals slot
        rotated.assign(3 * n, 0.f);
        GpuICPSequence::check(ctx, icpmi_deskew(ctx, cloud.features.data(), (int64_t)n, tRel.data(), &m, out.data(),
                                                cloud.getDescriptorByName("observationDirections").data.data(), rotated.data()));
        cloud.getDescriptorByName("observationDirections").data.swap(rotated);
    }
    cloud.features.swap(out);
}

void Mapper::applyInputFilters(DataPoints& inputInSensorFrame)
{
    inputFilters.apply(inputInSensorFrame, radiusFilter.get()); // radius filter first, then the `input:` chain
}

void Mapper::processInput(const DataPoints& filteredInputInSensorFrame, const Mat4& estimatedPose, const TimePoint& timeStamp)
{
    // One upload per scan when the map update can run on the resident map: the scan is moved by the prior, registered and --
    // if the policy asks for it -- moved by the correction and merged, all on the GPU (icpmi_register_prior /
    // icpmi_map_update_staged).  Offline only: an asynchronous update would race the next scan for the staged buffer.
    // (a reading with `simpleSensorNoise` takes the host-pointer path below: icpmi_register_prior does not carry the noise row that
    // ErrorMinimizer::getOverlap() then needs, Mapper.cpp:219)
    if (!isOnline && !icp.chainNeedsReadingNormals() && !icp.hasReadingFilters() && !icp.readsReadingDescriptor() &&
        !filteredInputInSensorFrame.descriptorExists("simpleSensorNoise") &&
        map.canStageScan(filteredInputInSensorFrame, mapPostFilters, &estimatedPose)) {
        const bool bootstrap = map.isLocalPointCloudEmpty();
        Mat4 correction;
        lastScanGrewMap = false;
        lastUpdMs = 0.0;
        const auto tReg = std::chrono::steady_clock::now();
        {
            std::lock_guard<std::mutex> g(icpMapLock);
            lastSeenMapVersion = map.icpMapVersion();
            correction = icp.registerWithPrior(filteredInputInSensorFrame, estimatedPose); // identity while there is no map
            lastScoreValid = false;
            if (scoreRegistrations && !bootstrap && icp.hasMap()) { lastScore = icp.residualStaged(correction); lastScoreValid = true; }
            keepLocalizability(!bootstrap && icp.hasMap());
        }
        lastCorrectionMat = bootstrap ? Mat4::identity() : correction;
        lastRegMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tReg).count();
        const Mat4 correctedPose = bootstrap ? estimatedPose : correction * estimatedPose;
        map.updatePose(correctedPose);
        if (bootstrap || mapUpdateIsDue(timeStamp, correctedPose, icp.errorMinimizer->getOverlap())) {
            const auto tUpd = std::chrono::steady_clock::now();
            struct UpdClock { const std::chrono::steady_clock::time_point t0; double& out; ~UpdClock() { out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } updClock{tUpd, lastUpdMs};
            lastTimeMapWasUpdated = timeStamp;
            lastPoseWhereMapWasUpdated = correctedPose;
            lastScanGrewMap = true;
            if (map.canStageScan(filteredInputInSensorFrame, mapPostFilters, &correctedPose))
                map.updateLocalPointCloudStaged(filteredInputInSensorFrame, bootstrap ? Mat4::identity() : correction, correctedPose, mapPostFilters);
            else { // paging in updatePose changed the picture (e.g. the local cloud was emptied): the host path
                DataPoints inMap = transformation.compute(filteredInputInSensorFrame, estimatedPose);
                if (!bootstrap) inMap = transformation.compute(inMap, correction);
                map.updateLocalPointCloud(inMap, correctedPose, mapPostFilters);
            }
        }
        { std::lock_guard<std::mutex> g(poseLock); pose = correctedPose; }
        { std::lock_guard<std::mutex> g(trajectoryLock); trajectory.addPose(correctedPose, timeStamp); }
        return;
    }

    // scan into the map frame by the prior; ICP then returns a correction expressed in the map frame
    DataPoints scanInMap = transformation.compute(filteredInputInSensorFrame, estimatedPose);
    const bool bootstrap = map.isLocalPointCloudEmpty(); // nothing to register against: the prior is the pose
    Mat4 correction = Mat4::identity();
    lastScanGrewMap = false;
    lastUpdMs = 0.0;
    const auto tReg = std::chrono::steady_clock::now();
    lastScoreValid = false;
    lastLocalizabilityValid = false;
    if (!bootstrap) {
        std::lock_guard<std::mutex> g(icpMapLock);
        lastSeenMapVersion = map.icpMapVersion();
        correction = icp(scanInMap);
        if (scoreRegistrations && icp.hasMap()) { lastScore = icp.residual(scanInMap, correction); lastScoreValid = true; }
        keepLocalizability(icp.hasMap());
    }
    lastCorrectionMat = correction;
    lastRegMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tReg).count();
    const Mat4 correctedPose = bootstrap ? estimatedPose : correction * estimatedPose;
    map.updatePose(correctedPose);
    const auto tUpd = std::chrono::steady_clock::now();
    if (bootstrap) { growMap(scanInMap, correctedPose, timeStamp); lastScanGrewMap = true; }
    else if (mapUpdateIsDue(timeStamp, correctedPose, icp.errorMinimizer->getOverlap())) {
        growMap(transformation.compute(scanInMap, correction), correctedPose, timeStamp);
        lastScanGrewMap = true;
    }
    if (lastScanGrewMap) lastUpdMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tUpd).count(); // (online: the hand-off only)

    // surface an exception of a finished asynchronous update here, like the reference's future.get()
    if (mapUpdateFuture.valid() && mapUpdateFuture.wait_for(std::chrono::milliseconds(1)) == std::future_status::ready) mapUpdateFuture.get();
    { std::lock_guard<std::mutex> g(poseLock); pose = correctedPose; }
    { std::lock_guard<std::mutex> g(trajectoryLock); trajectory.addPose(correctedPose, timeStamp); }
}

SweepRegistration Mapper::processSweep(const DataPoints& filteredInputInSensorFrame, const Mat4& estimatedPoseBegin, const Mat4& estimatedPoseEnd,
                                       const TimePoint& timeStamp, const SweepOptions& opts)
{
    const int64_t stampNs = (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(timeStamp.time_since_epoch()).count();
    std::vector<float> tRel;
    icpmi_sweep_options o;
    icpmi_sweep_options_default(&o);
    o.time_unit_s = sweepPointTimes(filteredInputInSensorFrame, stampNs, opts.timeField, opts.timeUnit, "processSweep", tRel);
    o.begin_s = opts.beginS; o.end_s = opts.endS;
    o.max_iterations = opts.maxIterations; o.min_step_rot = opts.minStepRot; o.min_step_trans = opts.minStepTrans;
    o.lambda_rot = opts.lambdaRot; o.lambda_trans = opts.lambdaTrans;
    const bool bootstrap = map.isLocalPointCloudEmpty(); // nothing to register against: the priors are the motion
    SweepRegistration reg;
    lastScanGrewMap = false;
    lastUpdMs = 0.0;
    lastScoreValid = false;
    lastLocalizabilityValid = false;
    const auto tReg = std::chrono::steady_clock::now();
    {
        std::lock_guard<std::mutex> g(icpMapLock);
        if (!bootstrap) lastSeenMapVersion = map.icpMapVersion();
        // (an empty reading, or no map on the handle yet: the call answers with the priors and their double form)
        DataPoints none(0);
        reg = icp.registerSweep(bootstrap ? none : filteredInputInSensorFrame, bootstrap ? std::vector<float>() : tRel, estimatedPoseBegin, estimatedPoseEnd, o);
    }
    lastRegMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tReg).count();
    // the cloud as seen from the end pose under that motion
    DataPoints deskewed = filteredInputInSensorFrame;
    SweepMotion motion;
    motion.stampNs = {stampNs + (int64_t)std::llround(opts.beginS * 1e9), stampNs + (int64_t)std::llround(opts.endS * 1e9)};
    for (int k = 0; k < 2; ++k) {
        std::array<double, 7> p;
        std::copy(reg.stats.pose7 + 7 * k, reg.stats.pose7 + 7 * k + 7, p.begin());
        motion.pose.push_back(p);
    }
    DeskewOptions dopts;
    dopts.timeField = opts.timeField; dopts.timeUnit = opts.timeUnit; dopts.extrapolate = true;
    dopts.refS = 1e-9 * (double)(motion.stampNs[1] - stampNs);
    deskewSweep(icp.handle(), deskewed, motion, timeStamp, dopts);
    // ... and from here on processInput's host path for that cloud at the end pose, the registration already done
    const Mat4 correctedPose = reg.end;
    lastCorrectionMat = Mat4::identity();
    const DataPoints scanInMap = transformation.compute(deskewed, correctedPose);
    map.updatePose(correctedPose);
    const auto tUpd = std::chrono::steady_clock::now();
    const float overlap = bootstrap ? 0.f : reg.stats.weighted_point_used_ratio;
    if (bootstrap || mapUpdateIsDue(timeStamp, correctedPose, overlap)) { growMap(scanInMap, correctedPose, timeStamp); lastScanGrewMap = true; }
    if (lastScanGrewMap) lastUpdMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tUpd).count();
    if (mapUpdateFuture.valid() && mapUpdateFuture.wait_for(std::chrono::milliseconds(1)) == std::future_status::ready) mapUpdateFuture.get();
    { std::lock_guard<std::mutex> g(poseLock); pose = correctedPose; }
    { std::lock_guard<std::mutex> g(trajectoryLock); trajectory.addPose(correctedPose, timeStamp); }
    return reg;
}

// the degeneracy report of the registration that just ran (registered = one did), for getLocalizability() and the map-update veto
void Mapper::keepLocalizability(bool registered)
{
    lastLocalizabilityValid = registered && icp.hasLocalizability();
    if (lastLocalizabilityValid) lastLocalizabilityReport = icp.errorMinimizer->getLocalizability();
}

icpmi_localizability Mapper::getLocalizability() const
{
    if (!lastLocalizabilityValid) throw std::runtime_error("Mapper::getLocalizability: the last processInput left no report (degeneracyThreshold is 0, or no scan was registered)");
    return lastLocalizabilityReport;
}

Relocalization Mapper::relocalize(const DataPoints& inputInSensorFrame, const std::vector<Mat4>& candidates, const TimePoint& timeStamp,
                                  const RelocalizeOptions& options)
{
    DataPoints scan = inputInSensorFrame;
    applyInputFilters(scan);
    Relocalization found;
    {
        std::lock_guard<std::mutex> g(icpMapLock);
        found = icp.relocalize(scan, candidates, options);
    }
    { std::lock_guard<std::mutex> g(poseLock); pose = found.pose; }
    { std::lock_guard<std::mutex> g(trajectoryLock); trajectory.addPose(found.pose, timeStamp); }
    return found;
}

VoxelRelocalization Mapper::relocalizeVoxel(const DataPoints& inputInSensorFrame, const std::vector<Mat4>& candidates, const TimePoint& timeStamp,
                                            const RelocalizeVoxelOptions& options)
{
    DataPoints scan = inputInSensorFrame;
    applyInputFilters(scan);
    VoxelRelocalization found;
    {
        std::lock_guard<std::mutex> g(icpMapLock);
        found = icp.relocalizeVoxel(scan, candidates, options);
    }
    { std::lock_guard<std::mutex> g(poseLock); pose = found.pose; }
    { std::lock_guard<std::mutex> g(trajectoryLock); trajectory.addPose(found.pose, timeStamp); }
    return found;
}

GlobalRelocalization Mapper::relocalizeGlobal(const DataPoints& inputInSensorFrame, const std::vector<Rot9>& rotations, const TimePoint& timeStamp,
                                              const GlobalLocalizeOptions& options, const RelocalizeOptions& refine, const RelocalizeVoxelOptions& refineVoxel)
{
    DataPoints scan = inputInSensorFrame;
    applyInputFilters(scan);
    GlobalRelocalization found;
    {
        std::lock_guard<std::mutex> g(icpMapLock);
        found = icp.relocalizeGlobal(scan, rotations, options, refine, refineVoxel);
    }
    { std::lock_guard<std::mutex> g(poseLock); pose = found.pose; }
    { std::lock_guard<std::mutex> g(trajectoryLock); trajectory.addPose(found.pose, timeStamp); }
    return found;
}

bool Mapper::mapUpdateIsDue(const TimePoint& now, const Mat4& poseNow, float overlap) const
{
    if (!isMapping.load()) return false;
    // setMaxDegenerateDirectionsForUpdate: a scan whose registration left more directions unconstrained than that is not written into the map
    if (maxDegenerateForUpdate >= 0 && lastLocalizabilityValid && lastLocalizabilityReport.n_degenerate > maxDegenerateForUpdate) return false;
    const bool updateInFlight = isOnline && mapUpdateFuture.valid() && mapUpdateFuture.wait_for(std::chrono::milliseconds(0)) != std::future_status::ready;
    if (updateInFlight) return false;
    float travelled2 = 0.f;
    const int euclideanDim = is3D ? 3 : 2;                                   // Mapper.cpp:266-269: topRightCorner(euclideanDim, 1)
    for (int axis = 0; axis < euclideanDim; ++axis) {
        const float step = poseNow(axis, 3) - lastPoseWhereMapWasUpdated(axis, 3);
        travelled2 += step * step;
    }
    const float seconds = std::chrono::duration<float>(now - lastTimeMapWasUpdated).count();
    return updatePolicy.due(std::sqrt(travelled2), overlap, seconds);
}

void Mapper::growMap(const DataPoints& inputInMapFrame, const Mat4& poseNow, const TimePoint& now)
{
    lastTimeMapWasUpdated = now;
    lastPoseWhereMapWasUpdated = poseNow;
    const bool inBackground = isOnline && !map.isLocalPointCloudEmpty(); // the very first map is built synchronously
    if (!inBackground) { map.updateLocalPointCloud(inputInMapFrame, poseNow, mapPostFilters); return; }
    // NIM_TEST_UPDATE_DELAY_MS (tests): the background update starts late, so that the next scans find it in flight -- they are
    // registered against the older map and start no update of their own (Mapper.cpp:257-260)
    static const int delayMs = [] { const char* e = std::getenv("NIM_TEST_UPDATE_DELAY_MS"); return e ? std::atoi(e) : 0; }();
    mapUpdateFuture = std::async(std::launch::async, [this, inputInMapFrame, poseNow] {
        if (delayMs > 0) std::this_thread::sleep_for(std::chrono::milliseconds(delayMs));
        map.updateLocalPointCloud(inputInMapFrame, poseNow, mapPostFilters);
    });
}

void Mapper::setMap(const DataPoints& newMap)
{
    map.setGlobalPointCloud(newMap);
    std::lock_guard<std::mutex> g(trajectoryLock);
    trajectory.clear();
}

Mat4 Mapper::getPose()
{
    std::lock_guard<std::mutex> g(poseLock);
    return pose;
}

Trajectory Mapper::getTrajectory()
{
    std::lock_guard<std::mutex> g(trajectoryLock);
    return trajectory;
}

} // namespace nim
