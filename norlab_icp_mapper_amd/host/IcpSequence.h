// IcpSequence.h -- `GpuICPSequence`: the four calls norlab_icp_mapper makes on its
// `PM::ICPSequence icp` member (Mapper.h:23), over the C ABI of include/icpmi.h:
//   loadFromYamlNode / setDefault   Mapper.cpp:72,77
//   setMap                          Map.cpp:111,178,528,581
//   operator()                      Mapper.cpp:213
//   errorMinimizer->getOverlap()    Mapper.cpp:219
// plus the registrar-created helpers the mapper uses next to it: RigidTransformation (Mapper.cpp:22,
// Map.cpp:14) and the DataPointsFilters of the shipped configuration (Mapper.cpp:27-31,82,92).
#pragma once
#include <array>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/icpmi.h"
#include "PointCloud.h"
#include "Yaml.h"

namespace nim {

class DataPointsFilters;

// YAML helpers of the chain loaders (IcpSequence.cpp; also the filter factory's): InvalidParameter on a key outside `known`;
// a `Name` / `Name: {params}` entry split into its name and parameters
void requireKnown(const yaml::Node& params, std::initializer_list<const char*> known, const std::string& who);
std::pair<std::string, yaml::Node> singleEntry(const yaml::Node& n, const std::string& what);
// the `matcher:` entry of an ICP chain (KDTreeMatcher | KDTreeVarDistMatcher) into cfg; maxDistField = the descriptor name of a
// KDTreeVarDistMatcher (default maxSearchDist), empty for KDTreeMatcher.  Needs no GPU.
void parseMatcher(const yaml::Node& matcher, icpmi_config& cfg, std::string& maxDistField, float* voxelSize = nullptr, // voxelSize: VoxelMatcher.voxelSize (the finest of voxelSizes), 0 for the others (null: VoxelMatcher is refused)
                  std::vector<float>* voxelSizes = nullptr);                                                            // voxelSizes: VoxelMatcher.voxelSizes, empty when the entry has none (null: the key is refused)
// the `errorMinimizer:` entry into cfg (minimizer, force2D / force4DOF, covariance, degeneracy options); planeEpsilon = the epsilon of a
// PlaneToPlaneErrorMinimizer (default 0.001; the others leave it alone); planeModel = ICPMI_PLANE_MODEL_SYMMETRIC under
// SymmetricPointToPlaneErrorMinimizer, which travels as ICPMI_MIN_PLANE_TO_PLANE (the others leave it alone).  Needs no GPU.
// intensity (may be null: the entry is still parsed and checked) = the photometric term of IntensityPointToPlaneErrorMinimizer, which travels as
// ICPMI_MIN_POINT_TO_PLANE with icpmi_set_intensity_weight (the others leave it alone: weight 0, off)
struct IntensityTerm {
    float weight = 0.f;                 // 1 - lambdaGeometric (icpmi_set_intensity_weight); 0: no such minimiser in the chain
    int knn = 10;                       // gradientKnn: neighbours of a map-side gradient (icpmi_set_map_intensity)
    std::string descName;               // descName: the 1-row descriptor both clouds carry (empty: no such minimiser)
};
// throws InvalidParameter unless a chain with VoxelMatcher (voxelSize > 0) has PlaneToPlaneErrorMinimizer (the GICP pair model) and no outlier filter
void checkVoxelChain(float voxelSize, int nOutlier, int minimizer, int planeModel);
void parseErrorMinimizer(const yaml::Node& node, icpmi_config& cfg, float& planeEpsilon, int& planeModel, IntensityTerm* intensity = nullptr);

// ---- relocalisation: one reading under many poses (include/icpmi.h: icpmi_residual_error_poses, icpmi_register_multistart) ----
// one icpmi_residual and one status per pose (a pose whose status is not ICPMI_OK keeps an empty residual); batched = the poses that
// went through the batched launches
struct PoseScores {
    std::vector<icpmi_residual> residual;
    std::vector<icpmi_status> status;
    int batched = 0;
    size_t size() const { return residual.size(); }
};
struct MultiStartResult {
    std::vector<Mat4> correction;       // per start, as registerWithPrior alone (identity where the status is not ICPMI_OK)
    std::vector<icpmi_stats> stats;
    std::vector<icpmi_status> status;
};
struct RelocalizeOptions {
    float minPairsRatio = 0.5f;         // a candidate needs pairs >= minPairsRatio * N
    int refine = 4;                     // how many of the best candidates are refined (at most 16)
    int kind = ICPMI_RES_CHAIN;
};
struct Relocalization {
    Mat4 pose = Mat4::identity();       // the winner's corrected pose: correction * candidate
    icpmi_residual residual{};          // ... scored under it
    int index = -1;                     // ... its index among the candidates
    PoseScores scores;                  // every candidate's first score
};
// The order in which a relocalisation prefers its candidates: status not ICPMI_OK or pairs < minPairsRatio * n (in double) are dropped, the
// rest come by sum_abs / pairs ascending (double), ties by the lower index.  Needs no GPU.
std::vector<int> rankCandidates(const PoseScores& scores, size_t n, float minPairsRatio);
// The start poses around `centre`: translations t + (dx, dy, 0), rotations Rz(dyaw) R, dx = halfX i / stepsX for i = -stepsX .. stepsX
// (likewise dy, dyaw; 0 steps: that axis stays), formed in double and rounded to float.  `centre` comes first, then yaw outermost, y, x
// innermost, each ascending: (2 stepsX + 1)(2 stepsY + 1)(2 stepsYaw + 1) poses.  Needs no GPU.
std::vector<Mat4> candidateGrid(const Mat4& centre, float halfX, float halfY, float halfYaw, int stepsX = 1, int stepsY = 1, int stepsYaw = 1);

// ---- relocalisation on the voxel path: poses scored by table lookup (include/icpmi.h: icpmi_voxel_score_poses) ----
// one icpmi_voxel_score and one status per pose (a pose that is not rigid keeps an empty score)
struct VoxelPoseScores {
    std::vector<icpmi_voxel_score> score;
    std::vector<icpmi_status> status;
    size_t size() const { return score.size(); }
};
struct RelocalizeVoxelOptions {
    int refine = 4;                     // how many of the best candidates are registered
    int level = 0;                      // the level the candidates are scored at (0: the coarsest of a schedule, the widest basin)
    float beta = 1.f;                   // l = exp(-beta / 2 d^T M d)
    float minPairsRatio = 0.f;          // a candidate needs pairs >= minPairsRatio * N
};
struct VoxelRelocalization {
    Mat4 pose = Mat4::identity();       // the winner's corrected pose: correction * candidate
    icpmi_voxel_score score{};          // ... scored under it at the finest level
    int index = -1;                     // ... its index among the candidates
    VoxelPoseScores scores;             // every candidate's first score
};
// The order in which a voxel relocalisation prefers its candidates: status not ICPMI_OK or pairs < minPairsRatio * n (in double) are
// dropped, the rest come by likelihood / n descending (double), ties by the lower index.  Needs no GPU.
std::vector<int> rankVoxelCandidates(const VoxelPoseScores& scores, size_t n, float minPairsRatio = 0.f);

// ---- global localisation: a search without candidates (include/icpmi.h: icpmi_global_localize) ----
using Rot9 = std::array<float, 9>;      // a rotation as the C call takes it: column-major 3 x 3
struct GlobalLocalizeOptions {
    float cellSize = 0.5f;              // s0: the finest cell, and the lattice's step
    int levels = 0;                     // occupancy levels, 1 .. 8 (0: automatic)
    float minScoreRatio = 0.f;          // a pose needs ceil(ratio * N) points in occupied cells
    int64_t maxNodes = 0;               // stop behind that many scored nodes with the best so far (0: no cap)
    int batch = 64;                     // nodes expanded per round
    bool hasBox = false;                // false: the map's bounding box
    std::array<double, 3> boxLo{{0, 0, 0}}, boxHi{{0, 0, 0}}; // the window in the map frame, metres
};
// Rz(2 pi i / steps) Ry(pitch) Rx(roll) for i = 0 .. steps - 1, formed in double -- every entry of a product summed left to right, Ry Rx
// first -- and rounded to float.  Needs no GPU.
std::vector<Rot9> yawRotations(int steps, double roll = 0.0, double pitch = 0.0);
// What GpuICPSequence::relocalizeGlobal returns: the search's result, and the refinement's with the found pose as its one candidate --
// `refined` on a KDTree chain, `refinedVoxel` on a VoxelMatcher chain (the other stays empty); pose is the one that holds
struct GlobalRelocalization {
    icpmi_global_localize_result search{};
    bool voxel = false;
    Relocalization refined;
    VoxelRelocalization refinedVoxel;
    Mat4 pose = Mat4::identity();
};

// What GpuICPSequence::registerSweep returns: the sensor's pose in the map at sweep begin and at sweep end, and the call's figures
// (include/icpmi.h: icpmi_sweep_result; stats.pose7 holds the two poses in double, as icpmi_sweep_motion takes them)
struct SweepRegistration {
    Mat4 begin = Mat4::identity(), end = Mat4::identity();
    icpmi_sweep_result stats{};
};

class GpuICPSequence {
public:
    struct ErrorMinimizerView {
        const GpuICPSequence* owner;
        float getOverlap() const { return owner->lastStats.sensor_noise_overlap >= 0.f ? owner->lastStats.sensor_noise_overlap : owner->lastStats.weighted_point_used_ratio; }
        float getPointUsedRatio() const { return owner->lastStats.point_used_ratio; }
        // PointToPlaneWithCovErrorMinimizer::getCovariance(): 6 x 6 column-major, (tx, ty, tz, alpha, beta, gamma), centred frame, of the
        // last registration (include/icpmi.h: icpmi_get_covariance); throws through check() when there is none
        std::array<float, 36> getCovariance() const;
        // degeneracyThreshold > 0 on the point-to-plane minimiser (not libpointmatcher's): which directions the last registration's last
        // counted iteration did not constrain (include/icpmi.h: icpmi_get_localizability); throws through check() when there is none
        icpmi_localizability getLocalizability() const;
        // ErrorMinimizer::getResidualError of `reading` against the map under the correction T, by the chain's minimizer: the sum over the
        // error elements of |p - q| (point-to-point) or |(p - q) . n| (point-to-plane) -- GpuICPSequence::residual(reading, T).sum_abs
        float getResidualError(const DataPoints& reading, const Mat4& T) const;
    };

    explicit GpuICPSequence(int device = 0);
    ~GpuICPSequence();
    GpuICPSequence(const GpuICPSequence&) = delete;
    GpuICPSequence& operator=(const GpuICPSequence&) = delete;

    void setDefault();                                 // PM::ICPSequence::setDefault
    void setVoxelMatcher(float size);                  // icpmi_set_voxel_matcher (0: off): VoxelMatcher on a PlaneToPlaneErrorMinimizer chain
    float getVoxelMatcher() const { return voxelSize; }
    void setVoxelSchedule(const std::vector<float>& sizes);   // icpmi_set_voxel_schedule: coarse-to-fine over 1 to 4 voxel sizes (empty: off)
    const std::vector<float>& getVoxelSchedule() const { return voxelSizes; }
    struct VoxelLevelReport { int iterations, pairsFirst, pairsLast; };
    std::vector<VoxelLevelReport> voxelScheduleReport() const; // icpmi_get_voxel_schedule_report: the last registration, level by level
    void loadFromYamlNode(const yaml::Node& icpNode);  // the `icp:` sub-tree
    bool setMap(const DataPoints& map);                // false on an empty cloud, state unchanged
    bool hasMap() const;
    Mat4 operator()(const DataPoints& reading);        // correction in the map frame
    const ErrorMinimizerView* errorMinimizer = &minimizerView;
    // How well `reading` (in the map frame by the prior, as for operator()) fits the map under the correction T: one matcher pass and the
    // chain's outlier filters on the device (include/icpmi.h: icpmi_residual_error).  The chain's reading filters are applied as operator()
    // applies them; `normals` and the rows the chain reads go with the reading.  Throws what operator() throws.  Leaves stats() alone.
    icpmi_residual residual(const DataPoints& reading, const Mat4& T, int kind = ICPMI_RES_CHAIN) const;
    // ... of the scan registerWithPrior left on the GPU (icpmi_residual_error_staged): no upload
    icpmi_residual residualStaged(const Mat4& T, int kind = ICPMI_RES_CHAIN) const;
    // residual(reading, T) for every T of `poses` in one call (icpmi_residual_error_poses): the reading filtered, uploaded, centred and
    // sorted once.  Errors of one pose are in its status; errors of the whole call throw what residual throws.
    PoseScores residuals(const DataPoints& reading, const std::vector<Mat4>& poses, int kind = ICPMI_RES_CHAIN) const;
    // the sensor-frame reading registered from every prior (at most 16) at once (icpmi_register_multistart): each start as
    // registerWithPrior alone.  Leaves no scan staged, no covariance and stats() alone.  The call carries the points alone: a chain that reads
    // the reading's normals (SurfaceNormalOutlierFilter) or a descriptor row (GenericDescriptor{source: reading}, maxDistField) is refused
    // with InvalidParameter, here and in relocalize (residuals serves such chains).
    MultiStartResult registerMultiStart(const DataPoints& readingInSensorFrame, const std::vector<Mat4>& priors);
    // Where is the sensor, given candidate poses?  Scores every candidate, drops and ranks them (rankCandidates), refines the best
    // options.refine with registerMultiStart, scores the refined poses once more and returns the winner by the same rule.
    // ConvergenceError when no candidate survives.
    Relocalization relocalize(const DataPoints& readingInSensorFrame, const std::vector<Mat4>& candidates, const RelocalizeOptions& options = RelocalizeOptions());

    // On a VoxelMatcher chain: the bounded likelihood of `reading` (with its `normals`) under every T of `poses` against the voxel table of
    // `level` (-1: the finest), one call (icpmi_voxel_score_poses).  The chain's reading filters are applied once.  Errors of one pose are in
    // its status; errors of the whole call throw.  Leaves stats() alone.
    VoxelPoseScores voxelScores(const DataPoints& reading, const std::vector<Mat4>& poses, int level = -1, float beta = 1.f) const;
    // On a VoxelMatcher chain: up to 16 readings, each with its `normals`, registered in one loop (icpmi_voxel_register_batch_dev after one
    // upload per reading); every reading as operator() registers it alone, bit for bit.  The chain's reading filters are applied once per
    // reading.  Errors of one reading are in its status; errors of the whole call throw in the C call's words.  stats() ends as the last
    // reading's; no covariance and no staged scan are left.
    MultiStartResult registerVoxelBatch(const std::vector<DataPoints>& readings);
    // ... one reading moved by every prior (at most 16) on the device and the moved readings registered in one loop
    // (icpmi_voxel_register_multistart): start s as RigidTransformation::compute(reading, priors[s]) followed by operator() alone.
    MultiStartResult registerVoxelMultiStart(const DataPoints& reading, const std::vector<Mat4>& priors);
    std::vector<VoxelLevelReport> voxelBatchReport(int member) const; // icpmi_get_voxel_batch_report: a member of the last of the two calls
    // Where is the sensor, given candidate poses -- on a VoxelMatcher chain: every candidate scored at options.level and ranked
    // (rankVoxelCandidates), the reading moved by each of the best options.refine registered by the chain as it is (the whole schedule, all
    // starts in one loop: registerVoxelMultiStart, chunks of 16), the refined poses scored at the finest level and ranked again.
    // ConvergenceError when nothing survives.
    VoxelRelocalization relocalizeVoxel(const DataPoints& reading, const std::vector<Mat4>& candidates, const RelocalizeVoxelOptions& options = RelocalizeVoxelOptions());

    // Where is the sensor, with no candidate at all?  The pose [R_k | mu + cellSize a] under which the most points of `reading` fall into
    // occupied cells of the map, over the lattice inside the box and the `rotations`, by branch and bound (icpmi_global_localize): exact,
    // no normals, no matcher.  The chain's reading filters are applied once.  found = 0 when nothing reaches minScoreRatio; errors throw.
    // Leaves stats() alone.
    icpmi_global_localize_result globalLocalize(const DataPoints& reading, const std::vector<Rot9>& rotations,
                                                const GlobalLocalizeOptions& options = GlobalLocalizeOptions()) const;
    // ... then the existing refinement with the found pose as its one candidate: relocalize, on a VoxelMatcher chain relocalizeVoxel.
    // ConvergenceError when the search finds nothing.
    GlobalRelocalization relocalizeGlobal(const DataPoints& reading, const std::vector<Rot9>& rotations,
                                          const GlobalLocalizeOptions& options = GlobalLocalizeOptions(), const RelocalizeOptions& refine = RelocalizeOptions(),
                                          const RelocalizeVoxelOptions& refineVoxel = RelocalizeVoxelOptions());

    // Sweep registration (include/icpmi.h: icpmi_register_sweep; not libpointmatcher's): the skewed scan in the sensor frame with its point
    // times tRel (one per point, in units of opts.time_unit_s from the scan's stamp) registered as a motion -- the two poses estimated by
    // the chain's matcher and outlier filters.  Point-to-plane chains without reading filters; throws what operator() throws.  Leaves
    // stats() and the staged scan alone; the covariance and the localizability report of the registration before it are dropped.
    SweepRegistration registerSweep(const DataPoints& scanInSensorFrame, const std::vector<float>& tRel, const Mat4& priorBegin, const Mat4& priorEnd,
                                    const icpmi_sweep_options& opts);
    icpmi_handle handle() const { return h; }          // for the operators that share the GPU context
    // Map::updateLocalPointCloud for the PointDistance chain on the resident map (icpmi_map_update_point_distance)
    void mapUpdatePointDistance(const DataPoints& inputInMapFrame, float minDist, int normalsKnn, std::vector<uint8_t>& keep, int64_t& appended,
                                int64_t& mapSize);
    DataPoints downloadMap() const;                    // the resident map (features + `normals` if it has them)
    // Mapper::processInput with the scan staged once on the GPU (icpmi_register_prior / icpmi_map_update_staged)
    Mat4 registerWithPrior(const DataPoints& scanInSensorFrame, const Mat4& prior);
    void mapUpdateStaged(const Mat4& correction, float minDist, int normalsKnn, std::vector<uint8_t>& keep, int64_t& appended, int64_t& mapSize);
    // Map::updateLocalPointCloud for a whole module chain + post filters on the resident map (icpmi_map_update_chain /
    // icpmi_map_update_chain_staged when `input` is null: the scan kept by registerWithPrior, moved by `correction`).
    // src[j] for j >= prefix: provenance of new map point j in [old map ; scan]; the first `prefix` points are untouched.
    // pose: the post filters run in the sensor frame (the map is moved by pose^-1 and back by pose, Map.cpp:523-525), on the device.
    void mapUpdateChain(const DataPoints* inputInMapFrame, const Mat4& correction, const std::string& scalarName, const DataPoints& scanDescriptors,
                        const Mat4& pose, const std::vector<icpmi_map_op>& ops, int nModules, std::vector<int32_t>& src, int64_t& prefix,
                        int64_t& mapSize, bool wantSrc = true); // wantSrc = false: no host-side descriptor needs the provenance vector
    void uploadMapScalar(const std::vector<float>& scalar);   // the tracked scalar descriptor of the resident map
    std::vector<float> downloadMapScalar() const;
    std::vector<float> downloadMapDensities() const;          // the `densities` row a resident SurfaceNormal{keepDensities: 1} step wrote
    int64_t residentMapSize() const;
    void setPlanar(bool on);                           // 2-D clouds (z == 0): planar minimisers and normals
    bool isPlanar() const { return planar; }
    const std::string& genericDescriptorName() const { return genericDescName; } // GenericDescriptorOutlierFilter.descName, or empty
    bool chainNeedsReadingNormals() const;             // SurfaceNormalOutlierFilter or PlaneToPlaneErrorMinimizer / SymmetricPointToPlaneErrorMinimizer in the chain
    // true when the chain filters the reading inside operator() (readingDataPointsFilters / readingStepDataPointsFilters):
    // the staged-scan path of Mapper::processInput hands the unfiltered scan to the GPU and must not be taken then
    bool hasReadingFilters() const;
    // referenceDataPointsFilters present: every map must pass through setMap (the resident map update rebuilds the index
    // from the device copy and would skip them)
    bool hasReferenceFilters() const { return referenceDataPointsFilters != nullptr; }
    const icpmi_stats& stats() const { return lastStats; }
    const icpmi_config& config() const { return cfg; }
    static void check(icpmi_handle h, icpmi_status s); // status -> exception mapping

    // The DataPointsFilters chains INSIDE the ICP object (PM::ICPChainBase: `readingDataPointsFilters`, applied to a copy of
    // the reading in its incoming frame at the top of operator(); `readingStepDataPointsFilters`, applied to a copy of the
    // reading at the top of every iteration -- every filter here gives the same result on the same input, so once;
    // `referenceDataPointsFilters`, applied to the centred copy of the map inside setMap).
    std::shared_ptr<DataPointsFilters> readingDataPointsFilters, readingStepDataPointsFilters, referenceDataPointsFilters;

private:
    void recreate();
    DataPoints filteredReading(const DataPoints& reading) const;
    PoseScores residualsFiltered(const DataPoints& reading, const std::vector<Mat4>& poses, int kind) const; // (the reading as the chain's filters left it)
    MultiStartResult multiStartFiltered(const DataPoints& reading, const std::vector<Mat4>& priors);
    VoxelPoseScores voxelScoresFiltered(const DataPoints& reading, const std::vector<Mat4>& poses, int level, float beta) const;
    MultiStartResult voxelMultiStartFiltered(const DataPoints& reading, const std::vector<Mat4>& priors);
    void requireBareReadingChain(const char* who) const;    // InvalidParameter for a chain that reads the reading's normals or descriptors
    icpmi_handle h = nullptr;
    icpmi_config cfg;
    icpmi_stats lastStats{};
    float planeEpsilon = 1e-3f;                        // PlaneToPlaneErrorMinimizer.epsilon (icpmi_set_plane_epsilon)
    float voxelSize = 0.f;                             // VoxelMatcher.voxelSize (icpmi_set_voxel_matcher; 0: a KDTree matcher)
    std::vector<float> voxelSizes;                     // VoxelMatcher.voxelSizes (icpmi_set_voxel_schedule; empty: voxelSize alone)
    int planeModel = ICPMI_PLANE_MODEL_GICP;           // ... and its pair model (icpmi_set_plane_pair_model): SymmetricPointToPlaneErrorMinimizer
    size_t stagedPoints = 0;                           // size of the scan kept on the GPU by registerWithPrior
    std::string genericDescName;                       // GenericDescriptorOutlierFilter.descName (empty: no such filter)
    std::string genericReadDescName;                   // ... of a filter with source: reading (the row goes to the device with every reading)
    std::string maxDistFieldName;                      // KDTreeVarDistMatcher: the reading's 1-row descriptor of search radii (empty: KDTreeMatcher)
    IntensityTerm intensity;                           // IntensityPointToPlaneErrorMinimizer (descName empty: not in the chain)
    void armReadingIntensity(const DataPoints& reading) const; // the reading's row of that descriptor, ahead of the call that takes the reading (one shot)
  public:
    bool readsReadingDescriptor() const { return !genericReadDescName.empty() || !maxDistFieldName.empty() || !intensity.descName.empty(); }
    const std::string& intensityDescriptorName() const { return intensity.descName; } // IntensityPointToPlaneErrorMinimizer.descName, or empty
    const std::string& maxDistField() const { return maxDistFieldName; } // KDTreeVarDistMatcher.maxDistField, or empty (KDTreeMatcher)
  private:
    bool planar = false;                               // 2-D mapping (is3D == false): icpmi_config::is_2d
    ErrorMinimizerView minimizerView{this};
    void keepCovariance();
    std::array<float, 36> covariance{};                // of the last registration, when the chain asks for it
    bool haveCovariance = false;
    icpmi_localizability localizability{};             // ... and its degeneracy report
    bool haveLocalizability = false;
  public:
    bool hasLocalizability() const { return haveLocalizability; } // the last registration left a report (Mapper's map-update veto reads it)
};

// PM::Transformation created with "RigidTransformation": features' = T * features, descriptors named
// "normals" / "observationDirections" rotated, everything else copied.
class RigidTransformation {
public:
    explicit RigidTransformation(icpmi_handle ctx) : h(ctx) {}
    DataPoints compute(const DataPoints& cloud, const Mat4& T) const;
private:
    icpmi_handle h;
};

// ---- DataPointsFilters used by the mapper and the shipped configuration -----------------------
class DataPointsFilter {
public:
    virtual ~DataPointsFilter() = default;
    virtual void inPlaceFilter(DataPoints& cloud) const = 0;
    // > 0 only for SurfaceNormalDataPointsFilter: lets Map run that post filter on the resident map
    virtual int surfaceNormalKnn() const { return 0; }
    // true when the filter can run as a step of icpmi_map_update_chain on the resident map: fills `op` and names the
    // scalar descriptor it reads (empty: none)
    virtual bool residentOp(icpmi_map_op& op, std::string& scalarName) const { (void)op; (void)scalarName; return false; }
    // true for per-point predicates (DistanceLimit, BoundingBox): a run of them is one icpmi_filter_points pass
    virtual bool pointFilter(icpmi_point_filter& f) const { (void)f; return false; }
    // true for the sensor-model filters (ObservationDirection, OrientNormals, Shadow, SimpleSensorNoise): per-point functions of the
    // position, the normal and a sensor position; a run of them is one icpmi_sensor_model pass
    virtual bool sensorStep(icpmi_sensor_step& s) const { (void)s; return false; }
    // false when two calls on the same cloud may differ (RandomSampling seeded from std::random_device): such a filter cannot
    // serve as a readingStepDataPointsFilter, which the accelerated loop applies once instead of once per iteration
    virtual bool repeatable() const { return true; }
    // true when the kept points get new coordinates (VoxelGrid's centroids): setMap then cannot put the caller's coordinates back
    virtual bool movesFeatures() const { return false; }
};

class DataPointsFilters {
public:
    DataPointsFilters() = default;
    // a YAML sequence of single-key maps, e.g. the `input:` and `post:` sections (Mapper.cpp:82,92)
    DataPointsFilters(const yaml::Node& seq, icpmi_handle ctx);
    // the chain in order; runs of per-point predicates (optionally starting with `leading`, the mapper's radius filter,
    // Mapper.cpp:187-191) go through one fused GPU pass and one compaction, and so do runs of sensor-model filters
    void apply(DataPoints& cloud, const DataPointsFilter* leading = nullptr) const;
    size_t size() const { return filters.size(); }
    std::vector<std::shared_ptr<DataPointsFilter>> filters;
    icpmi_handle ctx = nullptr;
};

std::shared_ptr<DataPointsFilter> createDataPointsFilter(const std::string& name, const yaml::Node& params, icpmi_handle ctx);

} // namespace nim
