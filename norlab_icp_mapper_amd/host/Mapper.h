// Mapper.h -- the orchestrator (reference: norlab_icp_mapper/Mapper.{h,cpp}): YAML configuration,
// input filters, the ICP call, map-update policy, pose / trajectory bookkeeping, optional asynchronous
// map update.  Same constructor arguments and public methods as the reference class.
#pragma once
#include <atomic>
#include <chrono>
#include <future>
#include <mutex>
#include <string>
#include <vector>

#include "IcpSequence.h"
#include "Map.h"
#include "MapperModule.h"

namespace nim {

using TimePoint = std::chrono::time_point<std::chrono::steady_clock>;

// Trajectory.{h,cpp}: poses + steady_clock stamps; save() writes the positions as features and the
// rotation columns as descriptors orientationX/Y/Z, the stamps as the int64 time row "t" (Trajectory.cpp:35-47)
class Trajectory {
public:
    explicit Trajectory(int dimension = 3) : dimension(dimension) {}
    void addPose(const Mat4& pose, TimePoint stamp) { poses.push_back(pose); stamps.push_back(stamp); }
    void clear() { poses.clear(); stamps.clear(); }
    size_t size() const { return poses.size(); }
    const Mat4& pose(size_t i) const { return poses[i]; }
    TimePoint stamp(size_t i) const { return stamps[i]; }
    void save(const std::string& filename) const;
private:
    int dimension;
    std::vector<Mat4> poses;
    std::vector<TimePoint> stamps;
};

// When the map is grown (`mapper: updateCondition:` of the YAML; reference defaults Mapper.h:19-20): parsed once into a
// tagged value instead of being re-interpreted from its string on every scan.
struct UpdatePolicy {
    enum Kind { Distance, Overlap, Delay } kind = Distance;
    float threshold = 1.0f; // metres travelled / overlap ratio / seconds, by kind
    static UpdatePolicy fromYaml(const yaml::Node& updateCondition); // throws yaml::Exception with the reference's messages
    bool due(float metresSinceUpdate, float overlap, float secondsSinceUpdate) const {
        return kind == Overlap ? overlap < threshold : (kind == Delay ? secondsSinceUpdate > threshold : metresSinceUpdate > threshold);
    }
};

// Sweep deskewing (include/icpmi.h: icpmi_deskew; the reference's wrapper does it in front of applyInputFilters, docs/UsingInRos.md:211-224).
// The sensor's motion over the sweep: poses (tx ty tz qx qy qz qw) of the sensor in a fixed frame at stamps in nanoseconds on the clock
// of the scans' TimePoint stamps.
struct SweepMotion {
    std::vector<int64_t> stampNs;
    std::vector<std::array<double, 7>> pose;
};
struct DeskewOptions {
    std::string timeField = "t";  // float descriptor of offsets from the scan's stamp, or else an int64 `times` row of absolute nanoseconds
    double timeUnit = 1e-9;       // seconds per unit of the float descriptor (the bundled scans' `t`: nanoseconds)
    int64_t roundToNs = 0;        // > 0: point times are rounded to multiples of it first (the wrapper's deskewing_round_to_nanosecs)
    bool extrapolate = false;     // false: a point time outside the motion's stamps is an error (tf2's ExtrapolationException)
    double refS = 0.0;            // the time the output is expressed at, seconds from the scan's stamp (0: the stamp itself)
};
// Sweep registration (include/icpmi.h: icpmi_register_sweep; not libpointmatcher's): the span of the sweep in seconds from the scan's stamp,
// where the point times are (as DeskewOptions), the iteration's limits (< 0: the chain's minDiff*) and the motion prior's weights
struct SweepOptions {
    double beginS = 0.0, endS = 0.1;
    std::string timeField = "t";
    double timeUnit = 1e-9;
    int maxIterations = 12;
    float minStepRot = -1.f, minStepTrans = -1.f;
    double lambdaRot = 0.0, lambdaTrans = 0.0;
};
// every point of the cloud moved to where the sensor saw it from at `stamp`: features by T(stamp)^-1 T(point time), `normals` and
// `observationDirections` by its rotation; every other descriptor and the `times` rows stay.  InvalidField when the cloud has neither
// a float descriptor nor an int64 time row called opts.timeField.
void deskewSweep(icpmi_handle ctx, DataPoints& inputInSensorFrame, const SweepMotion& motion, TimePoint stamp, const DeskewOptions& opts = DeskewOptions());

class Mapper {
public:
    Mapper(const std::string& configFilePath, bool is3D, bool isOnline, bool isMapping, bool saveMapCellsOnHardDrive, int device = 0);
    ~Mapper();

    // the call a host places in front of applyInputFilters when the sensor moved during the sweep (no reference analogue in the library:
    // the ROS wrapper does it, docs/UsingInRos.md:211-224)
    void deskew(DataPoints& inputInSensorFrame, const SweepMotion& motion, TimePoint stamp, const DeskewOptions& opts = DeskewOptions()) {
        deskewSweep(icp.handle(), inputInSensorFrame, motion, stamp, opts);
    }
    void applyInputFilters(DataPoints& inputInSensorFrame);                                   // Mapper.cpp:187-191
    void processInput(const DataPoints& inputInSensorFrame, const Mat4& estimatedPose, const TimePoint& timeStamp); // :194-238
    // processInput for a scan that is still skewed and whose motion within the sweep nobody knows: the two priors (the sensor's pose in the map
    // at opts.beginS and at opts.endS from the stamp) are refined by GpuICPSequence::registerSweep against the current map, the cloud is
    // deskewed to the end pose under the estimated motion (deskewSweep: `normals` and `observationDirections` follow), and the call goes on as
    // processInput does for that cloud at the end pose: paging, update policy, map update, trajectory.  On an empty map the priors are the
    // motion.  Point times as Mapper::deskew takes them.  Returns the motion it used.
    SweepRegistration processSweep(const DataPoints& filteredInputInSensorFrame, const Mat4& estimatedPoseBegin, const Mat4& estimatedPoseEnd,
                                   const TimePoint& timeStamp, const SweepOptions& opts = SweepOptions());
    // Relocalisation against the current map: the input filters are applied to a copy of the scan, GpuICPSequence::relocalize picks and
    // refines the best of `candidates`, and its pose becomes the mapper's (getPose(): what the next processInput starts from; the
    // trajectory gets it under `timeStamp`).  The map is NOT updated, and neither is anything the last processInput left
    // (lastRegistrationMapVersion(), lastResidual(), ...); Map::updatePose is not called either, so after a jump to a distant pose the map's
    // cells are paged by the next processInput, not here.  Throws what GpuICPSequence::relocalize throws; the pose then stays.
    Relocalization relocalize(const DataPoints& inputInSensorFrame, const std::vector<Mat4>& candidates, const TimePoint& timeStamp,
                              const RelocalizeOptions& options = RelocalizeOptions());
    // ... on a VoxelMatcher chain, by GpuICPSequence::relocalizeVoxel: the input filters, the current map, the pose set, no map update
    VoxelRelocalization relocalizeVoxel(const DataPoints& inputInSensorFrame, const std::vector<Mat4>& candidates, const TimePoint& timeStamp,
                                        const RelocalizeVoxelOptions& options = RelocalizeVoxelOptions());
    // ... with no candidate at all, by GpuICPSequence::relocalizeGlobal (the search over `rotations` and the lattice, then the refinement the
    // chain has): the input filters, the current map, the pose set, no map update
    GlobalRelocalization relocalizeGlobal(const DataPoints& inputInSensorFrame, const std::vector<Rot9>& rotations, const TimePoint& timeStamp,
                                          const GlobalLocalizeOptions& options = GlobalLocalizeOptions(), const RelocalizeOptions& refine = RelocalizeOptions(),
                                          const RelocalizeVoxelOptions& refineVoxel = RelocalizeVoxelOptions());
    DataPoints getMap() { return map.getGlobalPointCloud(); }
    long residentMapUpdates() const { return map.residentUpdateCount(); }
    size_t localMapSize() { return map.localSize(); }
    // online mode: blocks until the asynchronous map update in flight (Mapper.cpp:282) and every scheduled cell load / unload
    // (Map.cpp:35-57) are done.  No reference analogue; a replay that calls it after every processInput makes the online
    // pipeline reproduce the offline trajectory (the reference's online results depend on thread timing).
    void waitForPendingWork() { if (mapUpdateFuture.valid()) mapUpdateFuture.wait(); map.waitForPaging(); }
    void setMap(const DataPoints& newMap);
    bool getNewLocalMap(DataPoints& mapOut) { return map.getNewLocalPointCloud(mapOut); }
    Mat4 getPose();
    bool getIsMapping() const { return isMapping.load(); }
    void setIsMapping(bool v) { isMapping.store(v); }
    Trajectory getTrajectory();
    void setDefaultMapperModule();
    void loadYamlConfig(const std::string& configFilePath);
    void loadYamlConfigFromString(const std::string& text);
    const icpmi_stats& lastIcpStats() const { return icp.stats(); }
    const GpuICPSequence& icpSequence() const { return icp; } // (errorMinimizer->getCovariance() of the last registration)
    // Score every successful registration (off by default; no YAML key: the `mapper:` keys mirror the reference's): right after the ICP
    // call processInput evaluates the scan under the correction it got (GpuICPSequence::residualStaged on the one-upload path, residual
    // on the host path) and keeps the answer.  lastResidualValid(): the last processInput registered a scan and scored it.
    void setScoreRegistrations(bool on) { scoreRegistrations = on; }
    const icpmi_residual& lastResidual() const { return lastScore; }
    bool lastResidualValid() const { return lastScoreValid; }
    // degeneracyThreshold on the point-to-plane minimiser (no reference analogue): the report of the last processInput's registration
    // (include/icpmi.h: icpmi_get_localizability); throws std::runtime_error when that call registered nothing or the option is off
    icpmi_localizability getLocalizability() const;
    bool lastLocalizabilityIsValid() const { return lastLocalizabilityValid; }
    // -1 (default): never veto.  Otherwise a scan whose registration reported MORE degenerate directions than this is not written into
    // the map (the update policy is not even asked); its pose is published as always.
    void setMaxDegenerateDirectionsForUpdate(int n) { maxDegenerateForUpdate = n; }
    const Mat4& lastCorrection() const { return lastCorrectionMat; } // the correction of the last processInput's ICP call (identity: none ran)
    // the last processInput: version of the registration map it ran against (Map::icpMapVersion, read under the ICP lock) and
    // whether it started a map update -- what a replay needs to reproduce a free-running online run scan by scan
    long lastRegistrationMapVersion() const { return lastSeenMapVersion; }
    bool lastScanStartedMapUpdate() const { return lastScanGrewMap; }
    // wall time of the last processInput's two halves (offline mode; host clock around the calls, the GPU work is waited for inside them):
    // the ICP call (Mapper.cpp:213) and the map update it started (Map::updateLocalPointCloud, 0 when none was due).  Measurement only.
    double lastRegisterMs() const { return lastRegMs; }
    double lastMapUpdateMs() const { return lastUpdMs; }

private:
    void fillRegistrar();
    void rebuildRadiusFilter();
    void configureMapperSection(const yaml::Node& mapperNode);                        // the `mapper:` block, or an undefined node
    bool mapUpdateIsDue(const TimePoint& now, const Mat4& poseNow, float overlap) const; // Mapper.cpp:240-272
    void growMap(const DataPoints& inputInMapFrame, const Mat4& poseNow, const TimePoint& now); // Mapper.cpp:274-288

    GpuICPSequence icp;                 // first: the filters and modules share its GPU context
    std::mutex poseLock, trajectoryLock, icpMapLock;
    DataPointsFilters inputFilters, mapPostFilters;
    UpdatePolicy updatePolicy;
    bool is3D, isOnline;
    long lastSeenMapVersion = 0;
    bool lastScanGrewMap = false;
    double lastRegMs = 0.0, lastUpdMs = 0.0;
    bool scoreRegistrations = false, lastScoreValid = false;
    icpmi_residual lastScore{};
    void keepLocalizability(bool registered);
    icpmi_localizability lastLocalizabilityReport{};
    bool lastLocalizabilityValid = false;
    int maxDegenerateForUpdate = -1;
    Mat4 lastCorrectionMat = Mat4::identity();
    std::atomic_bool isMapping;
    Map map;
    Mat4 pose = Mat4::identity();
    Trajectory trajectory;
    RigidTransformation transformation;
    std::shared_ptr<DataPointsFilter> radiusFilter;
    TimePoint lastTimeMapWasUpdated;
    Mat4 lastPoseWhereMapWasUpdated = Mat4::identity();
    mutable std::future<void> mapUpdateFuture;
    MapperModuleRegistrar registrar;
};

} // namespace nim
